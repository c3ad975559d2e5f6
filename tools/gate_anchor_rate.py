"""What the gate reference SLIDEO_GATE_ANCHOR (include/slideo_amd.h "Gate reference") costs and what it is for.  Three measurements,
each a run of its own:

  (rate)  default: the gated stream rate at the headline content (1080p, 500 pages, ORB-1000) on changed_gate_rate.py's lecture
          stream, 256 device-resident frames in 128-frame units, submit / collect: ANCHOR against PREVIOUS on the one library, in
          one process, alternated repeats, min / median / max; at --share 0.1 and 0.5 unless one is given.

              python tools/gate_anchor_rate.py [--share 0.1] [--frames 256] [--reps 5]

  (kernels)  --kernels none | all: gated units of 256 device-resident 640x360 frames (small images of 461x259) under PREVIOUS and
          ANCHOR, without and with a frame mask under SLIDEO_MASK_GATE, for a rocprofv3 --kernel-trace run of its own.  none: a held
          frame (no frame of a unit is flagged: the walk takes 64 frames per step); all: 256 unrelated frames (every frame is
          flagged: one step per frame).  --parse-trace <kernel trace csv> then prints per kernel and grid the count and the median
          duration, and frame_gram_kernel's share of the int8 matrix-core peak by the tiles it executes (gate_anchor_kernel and
          gate_anchor_state_kernel: the walk and state write of a library from before ANCHOR ran the settle's kernels at a cap of 0).

              rocprofv3 --kernel-trace --stats -d OUT -o none -- python tools/gate_anchor_rate.py --kernels none
              python tools/gate_anchor_rate.py --parse-trace OUT/.../none_kernel_trace.csv

  (use)   --use: a synthetic lecture stream of 640x360 frames (4 pages, ORB-500) in which a share of the page changes is an 8-, 16-
          or 32-frame linear fade and the rest hard cuts: under each rule the share of holds whose last frame stands behind a verdict
          for the page it shows (the last flagged frame at or before it got that page), and the frames sent through ORB.

Prints one line per measurement and a JSON line at the end."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NCPU = min(16, os.cpu_count() or 1)
UNIT = 128
INT8_PEAK = 5.0e15          # dense int8 matrix-core operations per second (2 x the BF16 peak of 2.5e15)


def parse_trace(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            key = (name, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0)), int(r.get("Grid_Size_Y", 1) or 1), int(r.get("Grid_Size_Z", 1) or 1))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    want = ("ssd_kernel", "ssd_masked_kernel", "gate_carried_ssd_kernel", "frame_gram_kernel", "gate_anchor_kernel", "gate_anchor_state_kernel", "gate_settle_kernel",
            "gate_settle_state_kernel", "gate_kernel", "direct_centre", "fill")
    for key, v in sorted(rows.items()):
        if not any(w in key[0] for w in want):
            continue
        med = float(np.median(v))
        out["%s grid %dx%dx%d" % key] = {"count": len(v), "median_us": med, "min_us": min(v), "max_us": max(v)}
        print("%-60s grid %7d x %3d x %3d  count %3d  median %9.1f us  min %9.1f  max %9.1f" % (key[0][-60:], key[1], key[2], key[3], len(v), med, min(v), max(v)))
        if "frame_gram_kernel" in key[0]:
            # executed MFMA tiles of 256 frames of 461x259: 4 x 4 wave tiles of 64 rows, 6 above the diagonal (4 products of 32 x 32) and
            # 4 on it (3 products), K = 358 272 bytes; 2 operations per multiply-add
            n, kp = 256, 358272
            t = n // 64
            ops = (t * (t - 1) // 2 * 4 + t * 3) * 32 * 32 * kp * 2
            share = ops / (med * 1e-6) / INT8_PEAK
            out["frame_gram_kernel int8 share"] = share
            print("    frame_gram_kernel at n = %d: %.2f Gop executed, %.1f Top/s, %.2f %% of the %.1f Pop/s int8 peak" % (n, ops / 1e9, ops / (med * 1e-6) / 1e12, 100 * share, INT8_PEAK / 1e15))
    print(json.dumps(out))


def stream(m, submit, n, unit):
    pend, got = [], []
    for i in range(0, n, unit):
        if len(pend) == m.max_in_flight():
            got.append(m.collect_changed(pend.pop(0)))
        pend.append(submit(i, min(unit, n - i)))
    got += [m.collect_changed(t) for t in pend]
    return tuple(np.concatenate([g[j] for g in got]) for j in range(3))


def kernels_main(case):
    import torch
    from slideo_amd import _capi, synth
    W, H, N = 640, 360, 256
    pages = synth.pages(4, 800, 450, threads=NCPU)
    if case == "none":
        base, _, _ = synth.frames(pages, 1, W, H, threads=NCPU)
        seq = np.repeat(base[:1], N, axis=0)
    else:
        seq = np.random.default_rng(3).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    d = torch.from_numpy(seq).cuda()
    mask = np.full((H, W), 255, np.uint8)
    mask[190:350, 390:630] = 0
    for masked in (False, True):
        m = _capi.Matcher(_capi.default_config(nfeatures=500, min_rating=12.0))
        m.add_pages(list(pages))
        m.finalize()
        if masked:
            m.set_frame_mask_scope(_capi.MASK_DETECT | _capi.MASK_GATE)
            m.set_frame_mask(mask)
        for ref in ("previous", "anchor"):
            m.set_gate_reference(ref)
            m.gate_reset_from_frame(seq[0])
            for _ in range(4):
                ch, _, _ = m.collect_changed(m.submit_changed_dev(d.data_ptr(), N, W, H))
            print("%s, %s, %s: %d of %d flagged in the last unit" % (case, "masked" if masked else "whole", ref, int(ch.sum()), N), flush=True)
        m.close()


def rate_main(a):
    import torch
    from slideo_amd import _capi, synth
    from changed_gate_rate import lecture, W, H
    N = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    fb = W * H * 3
    res = {"shape": "%d pages, %d 1080p device-resident frames, ORB-1000, units of %d" % (a.pages, N, UNIT), "shares": {}}
    for share in ([a.share] if a.share is not None else [0.1, 0.5]):
        d = torch.from_numpy(lecture(pages, N, share)).cuda()

        def run(ref):
            m.set_gate_reference(ref)                              # (resets the gate state: frame 0 is changed)
            return stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fb, c, W, H), N, UNIT)
        flags = {ref: run(ref)[0] for ref in ("previous", "anchor")}     # (warm: workspaces sized)
        r = {"changed_share": {k: float(v.mean()) for k, v in flags.items()}, "same_flags": bool(np.array_equal(flags["previous"], flags["anchor"]))}
        t = {"previous": [], "anchor": []}
        for _ in range(a.reps):                                    # (alternating, so that clock and thermal drift hit both alike)
            for ref in t:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(ref)
                t[ref].append(time.perf_counter() - t0)
        for ref in t:
            ms = sorted(x * 1e3 for x in t[ref])
            r[ref + "_ms"] = {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}
            print("share %.2f %-9s changed %.3f  min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s (of the stream)"
                  % (share, ref, r["changed_share"][ref], ms[0], float(np.median(ms)), ms[-1], N, N / (float(np.median(ms)) * 1e-3)), flush=True)
        p, q = r["previous_ms"], r["anchor_ms"]
        r["anchor_minus_previous_ms"] = q["median"] - p["median"]
        print("share %.2f: ANCHOR - PREVIOUS %.2f ms per %d frames (spread of PREVIOUS %.2f, of ANCHOR %.2f)"
              % (share, q["median"] - p["median"], N, p["max"] - p["min"], q["max"] - q["min"]), flush=True)
        res["shares"]["%.2f" % share] = r
        del d
    m.close()
    print(json.dumps(res))


def use_main(a):
    from slideo_amd import _capi, synth
    W, H = 640, 360
    rng = np.random.default_rng(20261019)
    pages = synth.pages(4, 800, 450, threads=NCPU)
    holds = a.holds
    base, truth, _ = synth.frames(pages, holds, W, H, threads=NCPU)
    m = _capi.Matcher(_capi.default_config(nfeatures=500, min_rating=12.0))
    m.add_pages(list(pages))
    m.finalize()
    res = {"shape": "%d holds of 640x360 frames, 4 pages, ORB-500; a fade: rint(A + (B - A) j / k)" % holds, "fades": {}}
    for k in (8, 16, 32):
        for fade_share in (0.0, 0.5, 1.0):
            seq, last, want = [], [], []
            for j in range(holds):
                if j > 0 and rng.random() < fade_share:
                    a64, b64 = base[j - 1].astype(np.float64), base[j].astype(np.float64)
                    seq += [np.rint(a64 + (b64 - a64) * s / k).astype(np.uint8) for s in range(1, k)]
                seq += [base[j]] * int(rng.integers(4, 13))
                last.append(len(seq) - 1)
                want.append(int(truth[j]))
            seq = np.stack(seq)
            r = {"frames": len(seq)}
            for ref in ("previous", "anchor"):
                m.set_gate_reference(ref)
                ch, _, v = m.match_changed_frames(seq)
                idx = np.nonzero(ch)[0]
                ok = 0
                for e, p in zip(last, want):
                    f = idx[idx <= e].max()
                    ok += int(v[f]["page_idx"] == p)
                r[ref] = {"holds_behind_their_page": ok / holds, "frames_through_orb": int(ch.sum())}
            res["fades"]["k%d_share%.1f" % (k, fade_share)] = r
            print("fade of %2d frames on %3.0f %% of the changes, %4d frames: holds behind a verdict for their page PREVIOUS %.3f ANCHOR %.3f; frames through ORB PREVIOUS %d ANCHOR %d"
                  % (k, 100 * fade_share, len(seq), r["previous"]["holds_behind_their_page"], r["anchor"]["holds_behind_their_page"],
                     r["previous"]["frames_through_orb"], r["anchor"]["frames_through_orb"]), flush=True)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=None)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", choices=["none", "all"], default=None)
    ap.add_argument("--parse-trace", default=None)
    ap.add_argument("--use", action="store_true")
    ap.add_argument("--holds", type=int, default=24)
    a = ap.parse_args()
    if a.parse_trace:
        return parse_trace(a.parse_trace)
    if a.kernels:
        return kernels_main(a.kernels)
    if a.use:
        return use_main(a)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    return rate_main(a)


if __name__ == "__main__":
    main()
