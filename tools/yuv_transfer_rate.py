"""Cost and use of the YUV transfer (include/slideo_amd.h "YUV transfer").  One process per mode:

  --kernels   128 1080p frames of random samples through the mask call (conversion + small images, no pages needed), three times
              under each of P010 (4:2:0), P210 (4:2:2) and 4:4:4 10-bit (NV24 layout, 10_msb), first under SDR — the nearest 10-bit
              kernels yuv420_to_bgr_desc_kernel<1> and two instances of yuv_sampled_to_bgr_kernel, the yardsticks — then under HLG:
              three instances of yuv_transfer_to_bgr_kernel.  Then the same under HLG on a SLIDE (a white page with dark text, the
              content the LDS broadcast is meant for).  All under (bt709, limited).  Run it under a profiler's kernel trace with
              statistics, in a run of its own: the yuv* rows are the time per 128 frames of each kernel.  It prints nothing but the
              wall times.
  --rates     host-fed match calls from PINNED memory, --frames 1080p P010 frames against --pages pages, ORB-1000, under the plain
              description ("bt709", "limited", "10_msb") and under ("hlg", 0), alternated, min / median / max.
  --use       the screen recording of tools/direct_rate.py, one frame per hold, encoded (numpy, float64: sRGB -> linear -> BT.2020 ->
              nits at 203 -> OETF -> 10-bit limited-range Y'CbCr, chroma the 2x2 mean) to HLG and to PQ P010.  Each read as today,
              ("bt709", "limited", "10_msb"); as today with a levels table learnt from those frames (levels_points at 1 % / 1 %); and
              under the transfer.  For each reading: the mean absolute BGR error against the source, the direct look-up's s_i of the
              full-screen holds against the page they show, the share reaching --t, the share of the holds the pipeline assigns to the
              page they show, and the re-projection similarity.

    python tools/yuv_transfer_rate.py --kernels | --rates | --use   [--frames 128] [--pages 100] [--reps 5] [--t 0.99]

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
from yuv_desc_rate import deck, dist, pinned, W, H, NCPU  # noqa: E402

KR, KB = 0.2627, 0.0593
SDR_DESC = ("bt709", "limited", "10_msb")


def signal(transfer, nits):
    """The inverse of the header's nits(e): HLG's OETF under the 1.2 system gamma of a 1000-nit display, ST 2084's inverse EOTF."""
    if transfer == "pq":
        m1, m2, c1, c2, c3 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0, 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
        y = (nits / 10000.0) ** m1
        return ((c1 + c2 * y) / (1.0 + c3 * y)) ** m2
    a, b, c = 0.17883277, 0.28466892, 0.55991073
    E = (nits / 1000.0) ** (1.0 / 1.2)
    return np.where(E <= 1.0 / 12.0, np.sqrt(3.0 * E), a * np.log(np.maximum(12.0 * E - b, 1e-300)) + c)


def encode_p010(frames, transfer, white_nits=203.0):
    """[n, H, W, 3] sRGB BGR -> [n, frame bytes] P010 (limited range, BT.2020 NCL, chroma the 2x2 mean) as uint8."""
    gamut = np.asarray(_capi.yuv_transfer_tables(transfer, "limited", white_nits)[1], np.float64) / 16384.0      # BT.2020 -> BT.709
    to2020 = np.linalg.inv(gamut)
    out = []
    for f in frames:
        c = f[..., ::-1].astype(np.float64) / 255.0                                                            # R G B
        lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
        e = signal(transfer, np.clip(lin @ to2020.T, 0.0, None) * white_nits)
        r, g, b = e[..., 0], e[..., 1], e[..., 2]
        y = KR * r + (1.0 - KR - KB) * g + KB * b
        sub = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
        q = lambda p: (np.clip(np.rint(p), 0, 1023).astype(np.uint16) << 6)
        Y = q(64.0 + 876.0 * y)
        U, V = q(512.0 + 896.0 * sub((b - y) / (2.0 * (1.0 - KB)))), q(512.0 + 896.0 * sub((r - y) / (2.0 * (1.0 - KR))))
        out.append(np.concatenate([Y.reshape(-1), np.stack([U, V], -1).reshape(-1)]).view(np.uint8))
    return np.stack(out)


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    rng = np.random.default_rng(1)
    n = 128
    forms = (("p010", "nv12", "420"), ("p210", "nv16", "422"), ("444-10", "nv24", "444"))
    slide = np.full((H, W, 3), 255, np.uint8)
    slide[200:880:40, 200:1700] = 30                                              # dark text lines on a white page
    for content in ("noise", "slide"):
        for transfer in (("sdr", "hlg") if content == "noise" else ("hlg",)):
            for name, fmt, sampling in forms:
                L, fb = _capi.yuv_layout(fmt, W, H, bytes_per_sample=2)
                if content == "noise":
                    buf = (rng.integers(0, 1024, (n, fb // 2), dtype=np.uint16) << 6).view(np.uint8).reshape(n, fb)
                else:
                    one = encode_p010(slide[None], "hlg")[0].view(np.uint16)
                    Y, C = one[:W * H].reshape(H, W), one[W * H:].reshape(H // 2, W // 2, 2)
                    if sampling != "420":
                        C = np.repeat(C, 2, axis=0)
                    if sampling == "444":
                        C = np.repeat(C, 2, axis=1)
                    frame = np.concatenate([Y.reshape(-1), C.reshape(-1)]).view(np.uint8)
                    assert frame.size == fb
                    buf = np.repeat(frame[None], n, axis=0)
                m.set_yuv_transfer("sdr")
                m.set_yuv_sampling("420")
                m.set_yuv_description(*SDR_DESC)
                m.set_yuv_sampling(sampling)
                m.set_yuv_transfer(transfer)
                for _ in range(3):
                    t0 = time.perf_counter()
                    m.changed_mask_yuv420(buf, W, H, L)
                    print("kernels: %-5s %-4s %-7s mask call of %d frames %.1f ms" % (content, transfer, name, n, (time.perf_counter() - t0) * 1e3), flush=True)
    m.close()


def rates(a):
    res = {"shape": "%d pages, %d 1080p P010 frames from pinned memory, ORB-1000" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)           # 32 distinct frames, cycled
    idx = np.arange(a.frames) % 32
    buf = pinned(encode_p010(frames, "hlg")[idx])
    L = _capi.yuv420_layout("nv12", W, H, bytes_per_sample=2)[0]
    m.set_yuv_description(*SDR_DESC)
    t = {"sdr": [], "hlg": []}
    for k in t:
        m.set_yuv_transfer(k)
        m.match_frames_yuv420(buf.numpy(), W, H, L)
    for _ in range(a.reps):
        for k in t:
            m.set_yuv_transfer(k)
            t0 = time.perf_counter()
            m.match_frames_yuv420(buf.numpy(), W, H, L)
            t[k].append(time.perf_counter() - t0)
    for k, v in t.items():
        r = mmm(v)
        res[k] = dict(r, frames_per_s=a.frames / (r["median"] * 1e-3))
        print("rates: %-4s min %.1f median %.1f max %.1f ms per %d frames = %.0f frames/s" % (k, r["min"], r["median"], r["max"], a.frames,
                                                                                          res[k]["frames_per_s"]), flush=True)
    m.close()
    print(json.dumps(res))


def use(a):
    res = {"shape": "%d pages, one frame per hold of %d 1080p frames of tools/direct_rate.py's screen recording, encoded to HLG and PQ P010 at "
                    "203 nits" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    seq, truth, starts = recording(m, pages, a.frames, 0.5, 0.25, 3)
    first, tr = starts, truth[starts]
    src = seq[first]
    fs = tr >= 0
    L = _capi.yuv420_layout("nv12", W, H, bytes_per_sample=2)[0]
    m.set_yuv_description(*SDR_DESC)
    for transfer in ("hlg", "pq"):
        yuv = encode_p010(src, transfer)
        for reading in ("as_today", "as_today_with_learnt_levels", "under_the_transfer"):
            m.set_frame_levels(None)
            m.set_yuv_transfer(transfer if reading == "under_the_transfer" else "sdr")
            points = None
            if reading == "as_today_with_learnt_levels":
                m.levels_begin()
                m.observe_frames_yuv420(yuv, W, H, L)
                lo, hi = m.levels_points(0.01, 0.01)
                m.levels_end()
                points = (list(lo), list(hi))
                m.set_frame_levels(_capi.frame_levels_lut(lo, hi))
            bgr = np.stack([m.yuv420_to_bgr(f, W, H, L) for f in yuv])
            if points:
                bgr = np.stack([m.levels_bgr(b) for b in bgr])
            err = np.abs(bgr.astype(np.int16) - src.astype(np.int16))
            smalls = np.stack([m.small_image(b) for b in bgr])
            ssd = m.page_small_ssd(smalls).astype(np.float64)
            npx = smalls.shape[1] * smalls.shape[2]
            rows = np.arange(len(first))
            s_truth = similarity(ssd[rows[fs], tr[fs]], npx)
            v = m.match_frames_yuv420(yuv, W, H, L)
            r = {"levels_points": points,
                 "bgr_abs_error_vs_source": {"mean": float(err.mean()), "p99": float(np.percentile(err, 99)), "max": int(err.max())},
                 "direct_s_i_full_screen_vs_shown_page": dist(s_truth),
                 "direct_nearest_page_is_the_truth_share": float((ssd.argmin(axis=1)[fs] == tr[fs]).mean()),
                 "direct_share_at_or_above_t": {"t": a.t, "share": float((s_truth >= a.t).mean())},
                 "pipeline_assigned_share": float((v["page_idx"] >= 0).mean()),
                 "pipeline_full_screen_assigned_to_truth_share": float((v["page_idx"][fs] == tr[fs]).mean()),
                 "pipeline_similarity_full_screen": dist(v["similarity"][fs & (v["page_idx"] >= 0)])}
            name = "%s %s" % (transfer, reading)
            res[name] = r
            for k, x in r.items():
                print("use: %-34s %-46s %s" % (name, k, x), flush=True)
        m.set_frame_levels(None)
        m.set_yuv_transfer("sdr")
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
