"""Use and cost of the frame mask's GATE scope (include/slideo_amd.h "Frame mask scope") at the headline content (500 pages,
ORB-1000, 256 device-resident 1080p frames, holds of geometric length, mean 1 / --share) with the speaker-sized inset of
tools/frame_mask_rate.py (20 % of the frame, bottom right) re-randomised on EVERY frame.  One process, alternated repeats,
min / median / max:

  use    the share of frames flagged changed and the stream's frames/s through gated submit / collect under SLIDEO_MASK_DETECT and
         under DETECT | GATE, beside the plain ungated rate; the inset as random binary texture, and as the held content +- A grey
         levels for each A of --amplitudes (where does the unmasked gate start to fail?)
  cost   the gated stream over the frames WITHOUT an inset: no mask against an all-255 mask under GATE (the same flags and kept
         frames, ssd_masked_kernel in place of ssd_kernel)
  map    the time of slideo_matcher_set_frame_mask under DETECT | GATE against DETECT alone: the validity map's build per mask

    python tools/gate_mask_rate.py [--share 0.1] [--frames 256] [--pages 500] [--reps 5] [--amplitudes 10,20,40,60,80,100,127]
                                   [--kernels-only] [--step-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: the clean gated stream twice without a mask and twice
under the all-255 GATE mask and nothing else, for a rocprofv3 --kernel-trace --stats run of its own (ssd_kernel and
ssd_masked_kernel on the same pairs).  --step-only: the clean gated stream without a mask alone, through no call an older library
lacks (SLIDEO_LIB_PATH: the parent commit's build, interleaved process by process as tools/ab_libs.sh does)."""
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
from changed_gate_rate import lecture, stream  # noqa: E402
from frame_mask_rate import inset_rect  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080
UNIT = 128


def mmm(ts):
    ms = sorted(x * 1e3 for x in ts)
    return {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--amplitudes", default="10,20,40,60,80,100,127")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    N = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    seq = lecture(pages, N, a.share)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    y0, x0 = inset_rect(W, H)
    hole = np.full((H, W), 255, np.uint8)
    hole[y0:, x0:] = 0
    full = np.full((H, W), 255, np.uint8)
    d_clean = torch.from_numpy(seq).cuda()
    fbb = W * H * 3
    res = {"shape": "%d pages, %d 1080p frames, ORB-1000, holds geometric with mean %.1f; inset %dx%d at (%d, %d), another one per frame"
                    % (a.pages, N, 1 / a.share, W - x0, H - y0, x0, y0)}

    def gated(d):
        m.gate_reset(None)
        out = []
        stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fbb, c, W, H), lambda t: out.append(m.collect_changed(t)), N, UNIT)
        return np.concatenate([o[0] for o in out])

    def plain(d):
        stream(m, lambda i, c: m.submit_dev(d.data_ptr() + i * fbb, c, W, H), m.collect, N, UNIT)

    def timed(runs, reps):
        """runs: name -> (prepare, run); `prepare` (the mask and scope of the run) stays outside the timed interval."""
        for prep, fn in runs.values():
            prep()
            fn()                                                                # (warm: workspaces sized, tables built)
        t = {k: [] for k in runs}
        for _ in range(reps):                                                   # (alternating, so that clock and thermal drift hit all alike)
            for k, (prep, fn) in runs.items():
                prep()
                t0 = time.perf_counter()
                fn()
                t[k].append(time.perf_counter() - t0)
        return {k: mmm(v) for k, v in t.items()}

    def report(name, r):
        print("%-28s min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s (of the stream)"
              % (name, r["min"], r["median"], r["max"], N, N / (r["median"] * 1e-3)), flush=True)

    if a.step_only:
        r = timed({"gated_clean_no_mask": (lambda: None, lambda: gated(d_clean))}, a.reps)["gated_clean_no_mask"]
        report("gated_clean_no_mask", r)
        res["gated_clean_no_mask_ms"] = r
        res["lib"] = os.environ.get("SLIDEO_LIB_PATH", "product")
        m.close()
        print(json.dumps(res))
        return

    def scope(s, mask):
        m.set_frame_mask_scope(s)
        m.set_frame_mask(mask)

    DET, BOTH = _capi.MASK_DETECT, _capi.MASK_DETECT | _capi.MASK_GATE
    if a.kernels_only:
        for mask, s in ((None, DET), (full, _capi.MASK_GATE)) * 2:
            scope(s, mask)
            gated(d_clean)
        m.close()
        return

    # ---- cost: the clean stream, no mask against the all-255 mask under GATE --------------------------------------------------
    def clean_run(masked):
        scope(_capi.MASK_GATE if masked else DET, full if masked else None)
        return gated(d_clean)

    f0, f1 = clean_run(False), clean_run(True)
    assert np.array_equal(f0, f1), "an all-255 mask under GATE must flag what no mask flags"
    res["clean_changed_share"] = float(f0.mean())
    c = timed({"no_mask": (lambda: scope(DET, None), lambda: gated(d_clean)),
               "all255_gate": (lambda: scope(_capi.MASK_GATE, full), lambda: gated(d_clean))}, a.reps)
    res["cost_ms"] = c
    for k, r in c.items():
        report("cost: gated, " + k, r)
    res["cost_all255_minus_no_mask_ms"] = c["all255_gate"]["median"] - c["no_mask"]["median"]
    res["cost_no_mask_spread_ms"] = c["no_mask"]["max"] - c["no_mask"]["min"]
    print("cost: all-255 GATE - no mask %.2f ms per %d frames; spread of no mask %.2f ms (changed share %.3f)"
          % (res["cost_all255_minus_no_mask_ms"], N, res["cost_no_mask_spread_ms"], res["clean_changed_share"]), flush=True)

    # ---- map: the validity map's build, per mask ------------------------------------------------------------------------------
    def set_time(s):
        m.set_frame_mask_scope(s)
        m.set_frame_mask(hole)                                                  # (warm)
        ts = []
        for _ in range(max(a.reps, 5)):
            t0 = time.perf_counter()
            m.set_frame_mask(hole)
            ts.append(time.perf_counter() - t0)
        return mmm(ts)

    res["set_mask_ms"] = {"detect": set_time(DET), "detect_gate": set_time(BOTH)}
    res["map_build_ms"] = res["set_mask_ms"]["detect_gate"]["median"] - res["set_mask_ms"]["detect"]["median"]
    res["n_valid"] = m.frame_mask_small()[1]
    print("set_frame_mask(1080p): DETECT median %.2f ms, DETECT|GATE median %.2f ms: the map's build %.2f ms per mask (n_valid %d)"
          % (res["set_mask_ms"]["detect"]["median"], res["set_mask_ms"]["detect_gate"]["median"], res["map_build_ms"], res["n_valid"]), flush=True)

    # ---- use: an inset that changes on every frame ----------------------------------------------------------------------------
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261017)
    ih, iw = H - y0, W - x0

    def with_inset(amplitude):
        d = d_clean.clone()
        if amplitude is None:                                                   # random binary texture (tools/frame_mask_rate.py)
            tex = torch.randint(0, 2, (N, ih, iw, 1), device="cuda", generator=gen, dtype=torch.uint8) * 255
            d[:, y0:, x0:] = tex
        else:                                                                   # the held content +- amplitude grey levels
            noise = torch.randint(-amplitude, amplitude + 1, (N, ih, iw, 3), device="cuda", generator=gen, dtype=torch.int16)
            d[:, y0:, x0:] = (d[:, y0:, x0:].to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
        return d

    res["use"] = {}
    amps = [None] + [int(x) for x in a.amplitudes.split(",") if x]
    for amp in amps:
        name = "texture" if amp is None else "pm%d" % amp
        d = with_inset(amp)
        scope(DET, hole)
        fd = gated(d)
        scope(BOTH, hole)
        fg = gated(d)
        u = {"changed_share_detect": float(fd.mean()), "changed_share_detect_gate": float(fg.mean()),
             "gate_flags_equal_clean": bool(np.array_equal(fg, f0))}
        print("inset %-8s changed share: DETECT %.3f   DETECT|GATE %.3f   (clean content %.3f; GATE flags equal the clean stream's: %s)"
              % (name, u["changed_share_detect"], u["changed_share_detect_gate"], res["clean_changed_share"], u["gate_flags_equal_clean"]), flush=True)
        if amp is None:
            t = timed({"gated_detect": (lambda: scope(DET, hole), lambda: gated(d)),
                       "gated_detect_gate": (lambda: scope(BOTH, hole), lambda: gated(d)),
                       "plain_all": (lambda: scope(DET, hole), lambda: plain(d))}, a.reps)
            u["ms"] = t
            for k, r in t.items():
                report("use: " + k, r)
            u["detect_over_detect_gate"] = t["gated_detect"]["median"] / t["gated_detect_gate"]["median"]
            u["plain_over_detect_gate"] = t["plain_all"]["median"] / t["gated_detect_gate"]["median"]
            print("use: DETECT / DETECT|GATE %.2fx   plain / DETECT|GATE %.2fx" % (u["detect_over_detect_gate"], u["plain_over_detect_gate"]), flush=True)
        res["use"][name] = u
        del d
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
