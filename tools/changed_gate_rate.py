"""Frame rate of the changed-frame gate (include/slideo_amd.h "Changed-frame gate") at the headline content (1080p, 500 pages,
ORB-1000) on a lecture-like sequence: holds of identical frames whose lengths are drawn from a fixed seed (geometric, mean
1 / --share), every hold showing the next frame of the synthetic stream.  One process, alternated repeats, min / median / max:

  (a) today's loop: changed_mask + match_kept_frames per batch of 64 (the batch slideo_amd/matching.py uses), pinned BGR and NV12
  (b) the gated synchronous call on the same host frames, per batch of 64
  (c) gated submit / collect on device-resident BGR and NV12 in 128-frame units
  (d) plain submit / collect of ALL frames (the cost of not gating)
  (e) plain submit / collect of the changed frames alone, pre-selected on the host (the floor for (c))

    python tools/changed_gate_rate.py [--share 0.1] [--frames 256] [--reps 3] [--kernels-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: (c) alone, twice, for a
rocprofv3 --kernel-trace --stats run of its own (gate_kernel, gather_frames_kernel beside yuv420_to_bgr_desc_kernel).

--devices 0,1,2 | 0,0 | all: the N-device group over these HIP ordinals instead (an ordinal may repeat: members then share a
device, which measures the mechanism and not scaling; all = every gfx950 device of the node).  Pinned BGR and NV12 host frames in
calls of 64 frames per member, at --share 0.1 and 0.5 unless one is given, the three forms as alternated repeats on the one library:

  (g) the gated group call (slideo_group_match_changed_frames_*)
  (p) the group's stop-and-go pair: changed_mask + match_kept_frames
  (u) the ungated group call over ALL frames (slideo_group_match_frames_*)

with the changed frames each member kept (shards are contiguous: a run of changed frames loads one member)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

from slideo_amd import _capi, synth  # noqa: E402
import yuv420_ref  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080
BATCH, UNIT = 64, 128


def lecture(pages, n, share, seed=20261016):
    rng = np.random.default_rng(seed)
    starts, i = [], 0
    while i < n:
        starts.append(i)
        i += int(rng.geometric(share))
    base, _, _ = synth.frames(pages, len(starts), W, H, threads=NCPU)
    seq = np.empty((n, H, W, 3), np.uint8)
    for j, s in enumerate(starts):
        seq[s:(starts[j + 1] if j + 1 < len(starts) else n)] = base[j]
    return seq


def stream(m, submit, collect, n, unit):
    pend = []
    for i in range(0, n, unit):
        if len(pend) == m.max_in_flight():
            collect(pend.pop(0))
        pend.append(submit(i, min(unit, n - i)))
    for t in pend:
        collect(t)


def shard(n, r, world):
    """slideo_amd/distributed.py shard_range: member r's block of a call of n frames."""
    base, rem = divmod(n, world)
    lo = r * base + min(r, rem)
    return lo, lo + base + (1 if r < rem else 0)


def group_main(a):
    devices = None if a.devices == "all" else [int(d) for d in a.devices.split(",")]
    N = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    g = _capi.Group(_capi.default_config(nfeatures=1000), devices)
    for i in range(0, a.pages, 50):
        g.add_pages(list(pages[i:i + 50]))
    g.finalize()
    members = len(g.devices)
    batch = BATCH * members
    shared = len(set(g.devices)) < members
    label = "%d members on devices %s%s" % (members, g.devices, " (members share a device: the mechanism, not scaling)" if shared else "")
    print(label, flush=True)
    L, fb = _capi.yuv420_layout("nv12", W, H)
    res = {"shape": "%d pages, %d 1080p frames, ORB-1000, calls of %d frames" % (a.pages, N, batch), "devices": g.devices, "label": label, "shares": {}}
    for share in ([a.share] if a.share is not None else [0.1, 0.5]):
        seq = lecture(pages, N, share)
        src = {"bgr": torch.from_numpy(seq).pin_memory().numpy(), "nv12": torch.from_numpy(yuv420_ref.frames_to_yuv(seq, L, fb)).pin_memory().numpy()}
        del seq

        def gated(kind):
            g.gate_reset(None)
            out = []
            for i in range(0, N, batch):
                f = src[kind][i:i + batch]
                out.append(g.match_changed_frames(f) if kind == "bgr" else g.match_changed_frames_yuv420(f, W, H, L))
            return out

        def pair(kind):
            prev, out = None, []
            for i in range(0, N, batch):
                f = src[kind][i:i + batch]
                c, _, prev = g.changed_mask(f, prev) if kind == "bgr" else g.changed_mask_yuv420(f, W, H, L, prev)
                idx = np.nonzero(c)[0]
                out.append((c, g.match_kept_frames(idx) if len(idx) else np.zeros(0, _capi.VERDICT_DTYPE)))
            return out

        def plain(kind):
            for i in range(0, N, batch):
                f = src[kind][i:i + batch]
                g.match_frames(f) if kind == "bgr" else g.match_frames_yuv420(f, W, H, L)

        r = {}
        runs = {}
        for kind in ("bgr", "nv12"):
            # (warm, and the check that both forms return one result) the flags and the verdicts of the changed frames
            got, want = gated(kind), pair(kind)
            kept = [0] * members
            for (c, _, v), (pc, pv) in zip(got, want):
                assert np.array_equal(c, pc) and v[c].tobytes() == pv.tobytes(), "the gated call and the pair disagree"
                for m in range(members):
                    lo, hi = shard(len(c), m, members)
                    kept[m] += int(c[lo:hi].sum())
            plain(kind)
            r["changed_share_%s" % kind] = sum(kept) / N
            r["kept_per_member_%s" % kind] = kept
            print("share %.2f %s: changed %.3f, kept per member %s" % (share, kind, sum(kept) / N, kept), flush=True)
            runs["g_gated_%s" % kind] = lambda k=kind: gated(k)
            runs["p_pair_%s" % kind] = lambda k=kind: pair(k)
            runs["u_plain_all_%s" % kind] = lambda k=kind: plain(k)
        t = {k: [] for k in runs}
        for _ in range(a.reps):                                                 # (alternating, so that clock and thermal drift hit all alike)
            for k, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                t[k].append(time.perf_counter() - t0)
        for k in runs:
            ms = sorted(x * 1e3 for x in t[k])
            r[k + "_ms"] = {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}
            print("share %.2f %-18s min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s (of the stream)"
                  % (share, k, ms[0], float(np.median(ms)), ms[-1], N, N / (float(np.median(ms)) * 1e-3)), flush=True)
        for kind in ("bgr", "nv12"):
            gm, pm, um = (r["%s_%s_ms" % (k, kind)] for k in ("g_gated", "p_pair", "u_plain_all"))
            r["g_minus_p_%s_ms" % kind] = gm["median"] - pm["median"]
            print("share %.2f %s: (g) - (p) %.2f ms (spread of (p) %.2f, of (g) %.2f)   (u) / (g) %.2fx"
                  % (share, kind, gm["median"] - pm["median"], pm["max"] - pm["min"], gm["max"] - gm["min"], um["median"] / gm["median"]), flush=True)
        res["shares"]["%.2f" % share] = r
    g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=None)
    ap.add_argument("--devices", default=None, help="the N-device group over these ordinals (0,1 | 0,0 | all)")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if a.devices:
        return group_main(a)
    a.share = 0.1 if a.share is None else a.share
    N = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    seq = lecture(pages, N, a.share)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    L, fb = _capi.yuv420_layout("nv12", W, H)
    nv12 = yuv420_ref.frames_to_yuv(seq, L, fb)
    pin_bgr = torch.from_numpy(seq).pin_memory().numpy()
    pin_nv = torch.from_numpy(nv12).pin_memory().numpy()
    d_bgr, d_nv = torch.from_numpy(seq).cuda(), torch.from_numpy(nv12).cuda()
    fbb = W * H * 3
    m.changed_mask(seq[:BATCH])                                                 # (warm) — the flags of the whole stream follow
    flags = {}
    for kind, frames, call in (("bgr", pin_bgr, lambda f, p: m.changed_mask(f, p)), ("nv12", pin_nv, lambda f, p: m.changed_mask_yuv420(f, W, H, L, p))):
        out, prev = [], None
        for i in range(0, N, BATCH):
            c, _, prev = call(frames[i:i + BATCH], prev)
            out.append(c)
        flags[kind] = np.concatenate(out)
    sel = {k: np.nonzero(v)[0] for k, v in flags.items()}
    d_sel = {"bgr": d_bgr[torch.from_numpy(sel["bgr"])].contiguous(), "nv12": d_nv[torch.from_numpy(sel["nv12"])].contiguous()}
    res = {"shape": "%d pages, %d 1080p frames, ORB-1000, holds geometric with mean %.1f" % (a.pages, N, 1 / a.share),
           "changed_share": {k: float(v.mean()) for k, v in flags.items()}}
    print("changed share: bgr %.3f nv12 %.3f" % (res["changed_share"]["bgr"], res["changed_share"]["nv12"]), flush=True)

    def pair(kind):
        prev = None
        for i in range(0, N, BATCH):
            if kind == "bgr":
                c, _, prev = m.changed_mask(pin_bgr[i:i + BATCH], prev)
            else:
                c, _, prev = m.changed_mask_yuv420(pin_nv[i:i + BATCH], W, H, L, prev)
            idx = np.nonzero(c)[0]
            if len(idx):
                m.match_kept_frames(idx)

    def gated_sync(kind):
        m.gate_reset(None)
        for i in range(0, N, BATCH):
            if kind == "bgr":
                m.match_changed_frames(pin_bgr[i:i + BATCH])
            else:
                m.match_changed_frames_yuv420(pin_nv[i:i + BATCH], W, H, L)

    def gated_stream(kind):
        m.gate_reset(None)
        if kind == "bgr":
            stream(m, lambda i, c: m.submit_changed_dev(d_bgr.data_ptr() + i * fbb, c, W, H), m.collect_changed, N, UNIT)
        else:
            stream(m, lambda i, c: m.submit_changed_yuv420_dev(d_nv.data_ptr() + i * fb, c, W, H, L, fb), m.collect_changed, N, UNIT)

    def plain_stream(kind, only_changed):
        t = (d_sel[kind] if only_changed else (d_bgr if kind == "bgr" else d_nv))
        n = t.shape[0]
        if kind == "bgr":
            stream(m, lambda i, c: m.submit_dev(t.data_ptr() + i * fbb, c, W, H), m.collect, n, UNIT)
        else:
            stream(m, lambda i, c: m.submit_yuv420_dev(t.data_ptr() + i * fb, c, W, H, L, fb), m.collect, n, UNIT)

    if a.kernels_only:
        for _ in range(2):
            gated_stream("bgr")
            gated_stream("nv12")
        m.close()
        return

    runs = {}
    for kind in ("bgr", "nv12"):
        runs["a_pair_%s" % kind] = lambda k=kind: pair(k)
        runs["b_gated_sync_%s" % kind] = lambda k=kind: gated_sync(k)
        runs["c_gated_stream_%s" % kind] = lambda k=kind: gated_stream(k)
        runs["d_plain_all_%s" % kind] = lambda k=kind: plain_stream(k, False)
        runs["e_plain_changed_%s" % kind] = lambda k=kind: plain_stream(k, True)
    for fn in runs.values():
        fn()                                                                    # (warm: workspaces sized, tables built)
    t = {k: [] for k in runs}
    for _ in range(a.reps):                                                     # (alternating, so that clock and thermal drift hit all alike)
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    for k in runs:
        ms = sorted(x * 1e3 for x in t[k])
        res[k + "_ms"] = {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}
        print("%-24s min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s (of the stream)"
              % (k, ms[0], float(np.median(ms)), ms[-1], N, N / (float(np.median(ms)) * 1e-3)), flush=True)
    for kind in ("bgr", "nv12"):
        med = {k[0]: res["%s_%s_ms" % (k, kind)]["median"] for k in ("a_pair", "b_gated_sync", "c_gated_stream", "d_plain_all", "e_plain_changed")}
        sp = res["a_pair_%s_ms" % kind]
        res["b_minus_a_%s_ms" % kind] = med["b"] - med["a"]
        res["a_spread_%s_ms" % kind] = sp["max"] - sp["min"]
        res["c_minus_e_%s_ms" % kind] = med["c"] - med["e"]
        print("%s: (b) - (a) %.2f ms (spread of (a) %.2f)   (c) - (e) %.2f ms   (d) / (c) %.2fx"
              % (kind, med["b"] - med["a"], sp["max"] - sp["min"], med["c"] - med["e"], med["d"] / med["c"]), flush=True)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
