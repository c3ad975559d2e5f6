"""What the gate memory (include/slideo_amd.h "Gate memory") costs and what it is for.  Measurements, each a run of its own:

  (kernels)  --kernels none | deferred | recalled [--memory M]: gated units of 256 device-resident 640x360 frames (small images of
          461x259) under SLIDEO_GATE_ANCHOR with a memory of M entries, for a rocprofv3 --kernel-trace run of its own.  none: a held
          frame (no frame is away: the walk takes 64 frames per step); deferred: 256 unrelated frames under the settle (0.99, 2**30)
          (every frame is away from everything and none still: one step per frame, everything deferred); recalled: two pictures in
          turn, frame by frame, with M >= 2 (every frame is away from the anchor and within the threshold of the other entry: one
          step per frame, everything recalled).  --parse-trace <kernel trace csv> then prints per kernel and grid the count and the
          median duration.

              rocprofv3 --kernel-trace --stats -d OUT -o none -- python tools/gate_memory_rate.py --kernels none --memory 16
              python tools/gate_memory_rate.py --parse-trace OUT/.../none_kernel_trace.csv

  (step)  --step: the same three gated units, timed (submit + collect of 256 frames, median of --reps, profiler off) under plain
          ANCHOR (M = 0; the recalled stream is then matched frame by frame and is left out) and M = 1, 16, 64 — no frame goes
          through ORB, so the time is the gate's.

  (stream)  --stream: a synthetic "revisit" lecture of --frames device-resident --width x --height frames (--pages pages,
          ORB --nfeatures): holds of 4 .. 12 frames; after a hold the stream cuts to the speaker camera and back to the same slide
          (share --camera), flips back one or two slides and forward again (share --flip), or moves on to the next slide; in
          --unit-frame units under ANCHOR and under a memory of 1, 4, 16 and 64: the frames sent through ORB, the recalled frames,
          the share of holds whose last frame stands behind a verdict for the page it shows (its ref's frame got that page), and
          the time per 256 frames (median of --reps).

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
    want = ("gate_carried_ssd_kernel", "frame_gram_kernel", "page_ssd_kernel", "gate_settle_kernel", "gate_settle_state_kernel", "gate_recall_kernel",
            "gate_memory_state_kernel", "direct_centre", "fill")
    for key, v in sorted(rows.items()):
        if not any(w in key[0] for w in want):
            continue
        med = float(np.median(v))
        out["%s grid %dx%dx%d" % key] = {"count": len(v), "median_us": med, "min_us": min(v), "max_us": max(v)}
        print("%-60s grid %7d x %3d x %3d  count %3d  median %9.1f us  min %9.1f  max %9.1f" % (key[0][-60:], key[1], key[2], key[3], len(v), med, min(v), max(v)))
    print(json.dumps(out))


def _unit_streams(W, H, N):
    from slideo_amd import synth
    pages = synth.pages(4, 800, 450, threads=NCPU)
    base, _, _ = synth.frames(pages, 2, W, H, threads=NCPU)
    held = np.repeat(base[:1], N, axis=0)
    rnd = np.random.default_rng(3).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    turn = np.stack([base[i % 2] for i in range(N)])
    return pages, base, {"none": (held, (0.0, 0)), "deferred": (rnd, (SETTLE, NEVER)), "recalled": (turn, (0.0, 0))}


def _gate_matcher(pages, settle, M):
    from slideo_amd import _capi
    m = _capi.Matcher(_capi.default_config(nfeatures=500, min_rating=12.0))
    m.add_pages(list(pages))
    m.finalize()
    m.set_gate_reference("anchor")
    m.set_gate_settle(*settle)
    m.set_gate_memory(M)
    return m


def kernels_main(case, M):
    import torch
    from slideo_amd import _capi
    W, H, N = 640, 360, 256
    pages, base, streams = _unit_streams(W, H, N)
    seq, settle = streams[case]
    if case == "recalled" and M < 2:
        raise SystemExit("--kernels recalled needs --memory >= 2")
    d = torch.from_numpy(seq).cuda()
    m = _gate_matcher(pages, settle, M)
    m.gate_reset_from_frame(base[0])
    for _ in range(5):
        ch, sim, _ = m.collect_changed(m.submit_changed_dev(d.data_ptr(), N, W, H))
        refs = m.last_gate_refs() if M else None
    rec = 0 if refs is None else int((~ch & (sim < np.float32(m.cfg.changed_similarity)) & (refs != _capi.GATE_REF_DEFERRED)).sum())
    print("%s, M %d: %d of %d matched, %d recalled, %d deferred in the last unit" % (
        case, M, int(ch.sum()), N, rec, 0 if refs is None else int((refs == _capi.GATE_REF_DEFERRED).sum())), flush=True)
    m.close()


def step_main(a):
    import torch
    W, H, N = 640, 360, 256
    pages, base, streams = _unit_streams(W, H, N)
    dev = {k: torch.from_numpy(v[0]).cuda() for k, v in streams.items()}
    runs = []
    for M in (0, 1, 16, 64):
        for case, (_, settle) in streams.items():
            if case == "recalled" and M < 2:
                continue
            runs.append((_gate_matcher(pages, settle, M), "%s, M %d" % (case, M), dev[case]))
    ms, res = {}, {}
    for rep in range(a.reps + 1):                                # (alternating; the first round warms: workspaces sized)
        for m, name, d in runs:
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
        print("%-18s min %.3f median %.3f max %.3f ms per %d frames" % (name, min(v), float(np.median(v)), max(v), N), flush=True)
    for m, _, _ in runs:
        m.close()
    print(json.dumps(res))


def revisit_stream(rng, n_slides, n_frames, camera, flip):
    """-> [(picture, hold length)]: picture >= 0 a slide, -1 the speaker camera."""
    holds, cur, total = [], 0, 0

    def hold(p):
        nonlocal total
        k = int(rng.integers(4, 13))
        holds.append((p, k))
        total += k

    hold(0)
    while total < n_frames:
        u = rng.random()
        if u < camera:
            hold(-1)
            hold(cur)
        elif u < camera + flip and cur >= 2:
            back = int(rng.integers(1, 3))
            hold(cur - back)
            hold(cur)
        else:
            cur = (cur + 1) % n_slides
            hold(cur)
    return holds


def stream_main(a):
    import torch
    from slideo_amd import _capi, synth
    W, H = a.width, a.height
    rng = np.random.default_rng(20261020)
    pages = synth.pages(a.pages, 800 * W // 640, 450 * H // 360, threads=NCPU)
    n_slides = min(a.slides, a.pages)
    base, truth, _ = synth.frames(pages, n_slides + 1, W, H, threads=NCPU)      # the last one stands for the speaker camera
    holds = revisit_stream(rng, n_slides, a.frames, a.camera, a.flip)
    pic, last, want = [], [], []
    for p, k in holds:
        pic += [p] * k
        last.append(len(pic) - 1)
        want.append(int(truth[p]) if p >= 0 else int(truth[n_slides]))
    pic = pic[:a.frames]
    keep = [j for j, e in enumerate(last) if e < a.frames]
    d_base = torch.from_numpy(base).cuda()
    d = d_base[torch.tensor([p if p >= 0 else n_slides for p in pic]).cuda()].contiguous()
    n, fb = len(pic), W * H * 3
    m = _capi.Matcher(_capi.default_config(nfeatures=a.nfeatures, min_rating=12.0))
    m.add_pages(list(pages))
    m.finalize()
    m.set_gate_reference("anchor")
    res = {"shape": "%d frames of %dx%d in units of %d, %d pages, ORB-%d; %d holds of 4 .. 12 frames over %d slides, camera %.2f, flip %.2f" % (
        n, W, H, a.unit, a.pages, a.nfeatures, len(keep), n_slides, a.camera, a.flip)}
    print(res["shape"], flush=True)

    def run(M):
        m.gate_reset(None)
        ch, v, refs, pend = [], [], [], []

        def collect():
            c, _, vv = m.collect_changed(pend.pop(0))
            ch.append(c); v.append(vv)
            refs.append(m.last_gate_refs() if M else np.zeros(len(c), np.int64))

        for i in range(0, n, a.unit):
            if len(pend) == m.max_in_flight():
                collect()
            pend.append(m.submit_changed_dev(d.data_ptr() + i * fb, min(a.unit, n - i), W, H))
        while pend:
            collect()
        return np.concatenate(ch), np.concatenate(v), np.concatenate(refs)

    for M in (0, 1, 4, 16, 64):
        m.set_gate_memory(M)
        ch, v, refs = run(M)                                      # (warm: workspaces sized)
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(M)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        idx = np.nonzero(ch)[0]
        ok = 0
        for j in keep:
            e = last[j]
            f = int(refs[e]) if M else int(idx[idx <= e].max())  # the matched frame the hold's last frame stands behind
            ok += int(f >= 0 and v[f]["page_idx"] == want[j])
        recalled = int((~ch & (refs >= 0) & (np.concatenate([[-3], refs[:-1]]) != refs)).sum()) if M else 0
        r = {"frames_through_orb": int(ch.sum()), "recalled": recalled, "holds_behind_their_page": ok / max(1, len(keep)),
             "ms_per_256_frames": float(np.median(ts)) * 1e3 * 256 / n, "ms_min": min(ts) * 1e3 * 256 / n, "ms_max": max(ts) * 1e3 * 256 / n}
        res["M%d" % M] = r
        print("M %2d: %3d of %d frames through ORB, %3d recalled, holds behind a verdict for their page %.3f, %.2f ms per 256 frames (min %.2f max %.2f)" % (
            M, r["frames_through_orb"], n, recalled, r["holds_behind_their_page"], r["ms_per_256_frames"], r["ms_min"], r["ms_max"]), flush=True)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", choices=["none", "deferred", "recalled"], default=None)
    ap.add_argument("--memory", type=int, default=16)
    ap.add_argument("--parse-trace", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--slides", type=int, default=24)
    ap.add_argument("--nfeatures", type=int, default=1000)
    ap.add_argument("--unit", type=int, default=128)
    ap.add_argument("--camera", type=float, default=0.4)
    ap.add_argument("--flip", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.parse_trace:
        return parse_trace(a.parse_trace)
    if a.kernels:
        return kernels_main(a.kernels, a.memory)
    if a.step:
        return step_main(a)
    if a.stream:
        return stream_main(a)
    ap.error("one of --kernels, --parse-trace, --step, --stream")


if __name__ == "__main__":
    main()
