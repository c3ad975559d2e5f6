"""What the group gate order CHAIN (include/slideo_amd.h "Group gate order") costs and what it is for.  One process, alternated
repeats, min / median / max; --devices 0,1 | 0,0 | all as tools/changed_gate_rate.py takes them (members that share a device measure
the mechanism, not scaling: the label says so).

  (a)  --previous: changed_gate_rate.py's lecture stream — 1080p frames against --pages pages, ORB-1000, holds geometric with mean
       1 / share, --frames frames in calls of 64 per member, host BGR and NV12 — under SLIDEO_GATE_PREVIOUS through the group's gated
       call under HALO and under CHAIN, at shares 0.1 and 0.5 unless --share is given: the halo upload (one extra frame per later
       member and call) saved, against the chain's wait.  Both orders return the same bytes (checked in the warm-up).

  (b)  --fades: gate_anchor_rate.py's / gate_settle_rate.py's fade lectures — --holds holds of 640x360 frames, 4 pages, ORB-500; a
       share of the page changes is an 8-, 16- or 32-frame linear fade — under ANCHOR and under the settle (0.99, 2**30), the chained
       group against the single matcher on the group's first device: the time of the stream in calls of 64 frames per member, the
       frames each member sent through ORB, and the time the later members blocked for the baton
       (slideo_group_gate_chain_waited, summed over the calls of a pass).  Both return the same bytes (checked in the warm-up).

Prints one line per measurement and a JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from changed_gate_rate import BATCH, H, NCPU, W, lecture, shard  # noqa: E402  (its imports: torch, slideo_amd, tests/yuv420_ref)
import torch  # noqa: E402
import yuv420_ref  # noqa: E402

from slideo_amd import _capi, synth  # noqa: E402

NEVER = 2 ** 30
SETTLE = 0.99


def _devices(a):
    return None if a.devices == "all" else [int(d) for d in a.devices.split(",")]


def _label(g):
    members = len(g.devices)
    shared = len(set(g.devices)) < members
    return "%d members on devices %s%s" % (members, g.devices, " (members share a device: the mechanism, not scaling)" if shared else "")


def _stats(ts):
    ms = sorted(x * 1e3 for x in ts)
    return {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}


def previous_main(a):
    N = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    g = _capi.Group(_capi.default_config(nfeatures=1000), _devices(a))
    for i in range(0, a.pages, 50):
        g.add_pages(list(pages[i:i + 50]))
    g.finalize()
    members = len(g.devices)
    batch = BATCH * members
    print(_label(g), flush=True)
    L, fb = _capi.yuv420_layout("nv12", W, H)
    res = {"shape": "%d pages, %d 1080p frames, ORB-1000, calls of %d frames, SLIDEO_GATE_PREVIOUS" % (a.pages, N, batch), "devices": g.devices,
           "label": _label(g), "shares": {}}
    for share in ([a.share] if a.share is not None else [0.1, 0.5]):
        seq = lecture(pages, N, share)
        src = {"bgr": torch.from_numpy(seq).pin_memory().numpy(), "nv12": torch.from_numpy(yuv420_ref.frames_to_yuv(seq, L, fb)).pin_memory().numpy()}
        del seq

        def gated(kind, order):
            g.set_gate_order(order)                                  # (resets the gate state)
            out, waited = [], 0.0
            for i in range(0, N, batch):
                f = src[kind][i:i + batch]
                out.append(g.match_changed_frames(f) if kind == "bgr" else g.match_changed_frames_yuv420(f, W, H, L))
                waited += sum(g.gate_chain_waited(r) for r in range(1, members)) if order == "chain" else 0.0
            return out, waited

        r, runs = {}, {}
        for kind in ("bgr", "nv12"):
            (halo, _), (chain, _) = gated(kind, "halo"), gated(kind, "chain")
            for x, y in zip(halo, chain):
                assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), "HALO and CHAIN disagree under PREVIOUS"
            r["changed_share_%s" % kind] = float(np.concatenate([c for c, _, _ in chain]).mean())
            for order in ("halo", "chain"):
                runs["%s_%s" % (order, kind)] = lambda k=kind, o=order: gated(k, o)
        t = {k: [] for k in runs}
        w = {k: [] for k in runs}
        for _ in range(a.reps):                                      # (alternating, so that clock and thermal drift hit all alike)
            for k, fn in runs.items():
                t0 = time.perf_counter()
                _, waited = fn()
                t[k].append(time.perf_counter() - t0)
                w[k].append(waited)
        for k in runs:
            r[k + "_ms"] = _stats(t[k])
            s = r[k + "_ms"]
            print("share %.2f %-12s min %.2f median %.2f max %.2f ms per %d frames%s" % (share, k, s["min"], s["median"], s["max"], N,
                  "   baton wait, later members, median %.2f ms" % (float(np.median(w[k])) * 1e3) if k.startswith("chain") else ""), flush=True)
            if k.startswith("chain"):
                r[k + "_baton_wait_ms"] = float(np.median(w[k])) * 1e3
        for kind in ("bgr", "nv12"):
            h, c = r["halo_%s_ms" % kind], r["chain_%s_ms" % kind]
            r["chain_minus_halo_%s_ms" % kind] = c["median"] - h["median"]
            print("share %.2f %s (changed %.3f): CHAIN - HALO %.2f ms (spread of HALO %.2f, of CHAIN %.2f)"
                  % (share, kind, r["changed_share_%s" % kind], c["median"] - h["median"], h["max"] - h["min"], c["max"] - c["min"]), flush=True)
        res["shares"]["%.2f" % share] = r
    g.close()
    print(json.dumps(res))


def fades_main(a):
    FW, FH = 640, 360
    rng = np.random.default_rng(20261019)
    pages = synth.pages(4, 800, 450, threads=NCPU)
    holds = a.holds
    base, truth, _ = synth.frames(pages, holds, FW, FH, threads=NCPU)
    cfg = _capi.default_config(nfeatures=500, min_rating=12.0)
    g = _capi.Group(cfg, _devices(a))
    g.add_pages(list(pages))
    g.finalize()
    g.set_gate_order("chain")
    members = len(g.devices)
    batch = BATCH * members
    m = _capi.Matcher(cfg, device=g.devices[0])
    m.add_pages(list(pages))
    m.finalize()
    print(_label(g), flush=True)
    modes = (("anchor", (0.0, 0)), ("settle", (SETTLE, NEVER)))
    res = {"shape": "%d holds of 640x360 frames, 4 pages, ORB-500, calls of %d frames; a fade: rint(A + (B - A) j / k); settle (%.2f, 2**30)"
                    % (holds, batch, SETTLE), "devices": g.devices, "label": _label(g), "fades": {}}
    for k in (8, 16, 32):
        for fade_share in (0.5, 1.0):
            seq = []
            for j in range(holds):
                if j > 0 and rng.random() < fade_share:
                    a64, b64 = base[j - 1].astype(np.float64), base[j].astype(np.float64)
                    seq += [np.rint(a64 + (b64 - a64) * s / k).astype(np.uint8) for s in range(1, k)]
                seq += [base[j]] * int(rng.integers(4, 13))
            seq = np.stack(seq)
            n = len(seq)
            r = {"frames": n}

            def run(obj):
                obj.gate_reset(None)
                out, waited = [], 0.0
                for i in range(0, n, batch):
                    out.append(obj.match_changed_frames(seq[i:i + batch]))
                    if obj is g:
                        waited += sum(g.gate_chain_waited(q) for q in range(1, members))
                return out, waited

            for name, settle in modes:
                for obj in (m, g):
                    obj.set_gate_settle(0.0, 0)
                    obj.set_gate_reference("anchor")
                    obj.set_gate_settle(*settle)
                (want, _), (got, _) = run(m), run(g)                 # (warm, and the check that both return one result)
                kept = [0] * members
                for i, (x, y) in enumerate(zip(want, got)):
                    assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), "the chained group and the single matcher disagree"
                    for q in range(members):
                        lo, hi = shard(len(y[0]), q, members)
                        kept[q] += int(y[0][lo:hi].sum())
                t, w = {"single": [], "chain": []}, []
                for _ in range(a.reps):
                    for key, obj in (("single", m), ("chain", g)):
                        t0 = time.perf_counter()
                        _, waited = run(obj)
                        t[key].append(time.perf_counter() - t0)
                        if obj is g:
                            w.append(waited)
                r[name] = {"frames_through_orb_per_member": kept, "single_ms": _stats(t["single"]), "chain_ms": _stats(t["chain"]),
                           "baton_wait_ms": _stats(w)}
                s, c, b = r[name]["single_ms"], r[name]["chain_ms"], r[name]["baton_wait_ms"]
                print("fade of %2d frames on %3.0f %% of the changes, %4d frames, %-6s: through ORB per member %s; single min %.2f median %.2f max %.2f ms; "
                      "chained group min %.2f median %.2f max %.2f ms; later members blocked for the baton min %.2f median %.2f max %.2f ms"
                      % (k, 100 * fade_share, n, name, kept, s["min"], s["median"], s["max"], c["min"], c["median"], c["max"], b["min"], b["median"], b["max"]),
                      flush=True)
            res["fades"]["k%d_share%.1f" % (k, fade_share)] = r
    m.close()
    g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0,0", help="the N-device group over these ordinals (0,1 | 0,0 | all)")
    ap.add_argument("--previous", action="store_true")
    ap.add_argument("--fades", action="store_true")
    ap.add_argument("--share", type=float, default=None)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--holds", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.previous:
        return previous_main(a)
    if a.fades:
        return fades_main(a)
    ap.error("one of --previous, --fades")


if __name__ == "__main__":
    main()
