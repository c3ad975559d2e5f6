"""What the gate settle (include/slideo_amd.h "Gate settle") costs and what it is for.  Measurements, each a run of its own:

  (kernels)  --kernels none | deferred | matched: gated units of 256 device-resident 640x360 frames (small images of 461x259) under
          plain ANCHOR and under a settle, for a rocprofv3 --kernel-trace run of its own: gate_carried_ssd_kernel's 256 + 1 pairs
          against the shipped SSD launch for the same 256 pairs in the ANCHOR path, and the walk.  none: a held frame (nothing is
          flagged: 64 frames per step); deferred: 256 unrelated frames under (0.99, 2**30) (every frame is away and none still:
          everything deferred, 64 frames per step); matched: the same frames under (0.99, 0) (every frame matched: one step per
          frame).  Plain ANCHOR and the settle run the same kernels (plain is the settle with a cap of 0), so a trace tells them apart
          only by gate_carried_ssd_kernel's grid, 256 against 257 rows: --only plain | settle runs one of the two alone.
          --parse-trace <kernel trace csv> then prints per kernel and grid the count and the median duration (gate_anchor_kernel and
          gate_anchor_state_kernel: the walk and state write of a library from before the two paths were merged).

              rocprofv3 --kernel-trace --stats -d OUT -o none -- python tools/gate_settle_rate.py --kernels none
              python tools/gate_settle_rate.py --parse-trace OUT/.../none_kernel_trace.csv

  (step)  --step: the same gated units, timed (submit + collect of 256 frames, median of --reps, profiler off), whole and under the
          mask: the held frame under plain ANCHOR and under the settle, and the unrelated frames under the settle (0.99, 2**30) —
          the three streams in which no frame goes through ORB, so the time is the gate's.

  (use)   --use: gate_anchor_rate.py's synthetic lecture streams of 640x360 frames (4 pages, ORB-500; a share of the page changes is
          an 8-, 16- or 32-frame linear fade, the rest hard cuts) under PREVIOUS, ANCHOR and the settle (0.99, 2**30): the share of
          holds whose last frame stands behind a verdict for the page it shows (the last matched frame at or before it got that
          page), the frames sent through ORB, and the time of the synchronous gated call scaled to 256 frames (median of --reps).

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
NEVER = 2 ** 30
SETTLE = 0.99


def parse_trace(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            key = (name, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0)), int(r.get("Grid_Size_Y", 1) or 1), int(r.get("Grid_Size_Z", 1) or 1))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    want = ("ssd_kernel", "ssd_masked_kernel", "gate_carried_ssd_kernel", "frame_gram_kernel", "gate_anchor_kernel", "gate_anchor_state_kernel",
            "gate_settle_kernel", "gate_settle_state_kernel", "direct_centre", "fill")
    for key, v in sorted(rows.items()):
        if not any(w in key[0] for w in want):
            continue
        med = float(np.median(v))
        out["%s grid %dx%dx%d" % key] = {"count": len(v), "median_us": med, "min_us": min(v), "max_us": max(v)}
        print("%-60s grid %7d x %3d x %3d  count %3d  median %9.1f us  min %9.1f  max %9.1f" % (key[0][-60:], key[1], key[2], key[3], len(v), med, min(v), max(v)))
    print(json.dumps(out))


def kernels_main(case, only=None):
    import torch
    from slideo_amd import _capi, synth
    W, H, N = 640, 360, 256
    pages = synth.pages(4, 800, 450, threads=NCPU)
    if case == "none":
        base, _, _ = synth.frames(pages, 1, W, H, threads=NCPU)
        seq = np.repeat(base[:1], N, axis=0)
    else:
        seq = np.random.default_rng(3).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    settle = (SETTLE, 0) if case == "matched" else (SETTLE, NEVER)
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
        m.set_gate_reference("anchor")
        for s in [x for x, name in (((0.0, 0), "plain"), (settle, "settle")) if only in (None, name)]:
            m.set_gate_settle(*s)
            m.gate_reset_from_frame(seq[0])
            for _ in range(4):
                ch, sim, _ = m.collect_changed(m.submit_changed_dev(d.data_ptr(), N, W, H))
            print("%s, %s, settle %s: %d of %d matched, %d deferred in the last unit" % (case, "masked" if masked else "whole", s, int(ch.sum()), N,
                                                                                         int(_capi.gate_deferred(ch, sim, m.cfg.changed_similarity).sum())), flush=True)
        m.close()


def step_main(a):
    import torch
    from slideo_amd import _capi, synth
    W, H, N = 640, 360, 256
    pages = synth.pages(4, 800, 450, threads=NCPU)
    base, _, _ = synth.frames(pages, 1, W, H, threads=NCPU)
    held = torch.from_numpy(np.repeat(base[:1], N, axis=0)).cuda()
    rnd = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (N, H, W, 3), dtype=np.uint8)).cuda()
    mask = np.full((H, W), 255, np.uint8)
    mask[190:350, 390:630] = 0
    res = {"lib": os.environ.get("SLIDEO_LIB_PATH", "product")}
    ms = {}
    runs = []
    for masked in (False, True):
        m = _capi.Matcher(_capi.default_config(nfeatures=500, min_rating=12.0))
        m.add_pages(list(pages))
        m.finalize()
        if masked:
            m.set_frame_mask_scope(_capi.MASK_DETECT | _capi.MASK_GATE)
            m.set_frame_mask(mask)
        m.set_gate_reference("anchor")
        for name, d, s in (("held, plain", held, (0.0, 0)), ("held, settle", held, (SETTLE, NEVER)), ("deferred, settle", rnd, (SETTLE, NEVER))):
            runs.append((m, "%s, %s" % ("masked" if masked else "whole", name), d, s))
    for rep in range(a.reps + 1):                                # (alternating; the first round warms: workspaces sized)
        for m, name, d, s in runs:
            m.set_gate_settle(*s)
            m.gate_reset_from_frame(base[0])
            m.collect_changed(m.submit_changed_dev(d.data_ptr(), N, W, H))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                ch, _, _ = m.collect_changed(m.submit_changed_dev(d.data_ptr(), N, W, H))
            torch.cuda.synchronize()
            if int(ch.sum()):
                raise SystemExit("%s: %d frames went through the pipeline" % (name, int(ch.sum())))
            if rep:
                ms.setdefault(name, []).append((time.perf_counter() - t0) * 1e3 / 4)
    for name, v in ms.items():
        res[name] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
        print("%-26s min %.3f median %.3f max %.3f ms per %d frames" % (name, min(v), float(np.median(v)), max(v), N), flush=True)
    for m in {id(r[0]): r[0] for r in runs}.values():
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
    modes = (("previous", "previous", (0.0, 0)), ("anchor", "anchor", (0.0, 0)), ("settle", "anchor", (SETTLE, NEVER)))
    res = {"shape": "%d holds of 640x360 frames, 4 pages, ORB-500; a fade: rint(A + (B - A) j / k); settle (%.2f, 2**30)" % (holds, SETTLE), "fades": {}}
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
            for name, ref, settle in modes:
                m.set_gate_settle(0.0, 0)
                m.set_gate_reference(ref)
                m.set_gate_settle(*settle)
                ch, _, v = m.match_changed_frames(seq)               # (warm: workspaces sized)
                ts = []
                for _ in range(a.reps):
                    m.gate_reset(None)
                    t0 = time.perf_counter()
                    m.match_changed_frames(seq)
                    ts.append(time.perf_counter() - t0)
                idx = np.nonzero(ch)[0]
                ok = 0
                for e, p in zip(last, want):
                    f = idx[idx <= e].max()
                    ok += int(v[f]["page_idx"] == p)
                r[name] = {"holds_behind_their_page": ok / holds, "frames_through_orb": int(ch.sum()),
                           "ms_per_256_frames": float(np.median(ts)) * 1e3 * 256 / len(seq)}
            res["fades"]["k%d_share%.1f" % (k, fade_share)] = r
            print("fade of %2d frames on %3.0f %% of the changes, %4d frames: holds behind a verdict for their page PREVIOUS %.3f ANCHOR %.3f settle %.3f; "
                  "frames through ORB %d / %d / %d; ms per 256 frames %.2f / %.2f / %.2f"
                  % (k, 100 * fade_share, len(seq), r["previous"]["holds_behind_their_page"], r["anchor"]["holds_behind_their_page"],
                     r["settle"]["holds_behind_their_page"], r["previous"]["frames_through_orb"], r["anchor"]["frames_through_orb"],
                     r["settle"]["frames_through_orb"], r["previous"]["ms_per_256_frames"], r["anchor"]["ms_per_256_frames"],
                     r["settle"]["ms_per_256_frames"]), flush=True)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", choices=["none", "deferred", "matched"], default=None)
    ap.add_argument("--only", choices=["plain", "settle"], default=None)
    ap.add_argument("--parse-trace", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--use", action="store_true")
    ap.add_argument("--holds", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.parse_trace:
        return parse_trace(a.parse_trace)
    if a.kernels:
        return kernels_main(a.kernels, a.only)
    if a.step:
        return step_main(a)
    if a.use:
        return use_main(a)
    ap.error("one of --kernels, --parse-trace, --step, --use")


if __name__ == "__main__":
    main()
