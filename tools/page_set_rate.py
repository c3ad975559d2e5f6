#!/usr/bin/env python3
"""Page sets on the configs[3]-sized deck (1000 synthetic 2001x1125 pages, ORB-1000) with 256 1080p frames in device memory:

  build_ms    the time slideo_matcher_create_page_set takes for sets of 50, 100, 500 and 1000 pages, after one warm-up build.  The
              call is synchronous (its last step waits for the stream), so this is the host wall time of the call: every kernel of
              the build plus the one count read-back and the host's tile shuffle.
  fps         frames/s of three cases, alternated in one process, three repeats each: the whole deck, a 100-page set, and a
              standalone matcher built from the same 100 pages (slideo_matcher_add_page_features).  The set's verdicts are checked
              against the standalone matcher's on every repeat (page indices mapped).

The last line of output is one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (frames in device memory)
from slideo_amd import _capi, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pages", type=int, default=1000)
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--calls", type=int, default=4, help="frame calls per timed case")
a = ap.parse_args()

PW, PH, FW, FH = 2001, 1125, 1920, 1080
t0 = time.time()
pages = synth.pages(a.pages, PW, PH, threads=16)
cfg = _capi.default_config(nfeatures=1000)
m = _capi.Matcher(cfg)
for i in range(0, a.pages, 50):
    m.add_pages(list(pages[i:i + 50]))
m.finalize()
S100 = list(range(0, a.pages, a.pages // 100))[:100]
frames, _, _ = synth.frames(pages[S100], a.frames, FW, FH, threads=16)
del pages
print("deck: %d pages, %d rows, %d distinct (%.0f s)" % (a.pages, m.descriptor_count, m.unique_descriptor_count, time.time() - t0), flush=True)

# ---- set build time ----
rng = np.random.default_rng(7)
m.release_page_set(m.create_page_set(S100))                    # warm-up (uploads finalize's host arrays once)
build = {}
for k in (50, 100, 500, 1000):
    k = min(k, a.pages)
    sel = np.sort(rng.choice(a.pages, k, replace=False))
    t = time.perf_counter()
    sid = m.create_page_set(sel)
    ms = (time.perf_counter() - t) * 1e3
    info = m.page_set_info(sid)
    build[str(k)] = dict(ms=round(ms, 2), rows=info["rows"], unique_rows=info["unique_rows"], mb=round(info["bytes"] / 2 ** 20, 1))
    m.release_page_set(sid)
    print("set of %4d pages: %8.2f ms  (%d rows, %d distinct)" % (k, ms, info["rows"], info["unique_rows"]), flush=True)

# ---- frame rates ----
sub = _capi.Matcher(cfg)
for p in S100:
    kp, desc = m.page_features(p)
    sub.add_page_features(PW, PH, kp, desc, m.page_small(p))
sub.finalize()
sid = m.create_page_set(S100)
d = torch.from_numpy(frames).cuda()
torch.cuda.synchronize()
n = a.frames


def run(matcher, set_id):
    if set_id is not None:
        matcher.use_page_set(set_id)
    v = matcher.match_frames_dev(d.data_ptr(), n, FW, FH)      # warm-up call of the case
    t = time.perf_counter()
    for _ in range(a.calls):
        v = matcher.match_frames_dev(d.data_ptr(), n, FW, FH)
    dt = time.perf_counter() - t
    return n * a.calls / dt, v


cases = {"deck": (m, 0), "set100": (m, sid), "standalone100": (sub, None)}
fps = {k: [] for k in cases}
S = np.array(S100, np.int32)
for r in range(a.repeats):
    out = {}
    for name, (mm, s) in cases.items():
        f, out[name] = run(mm, s)
        fps[name].append(round(f, 1))
    vs = out["standalone100"].copy()
    vs["page_idx"] = np.where(vs["page_idx"] >= 0, S[np.maximum(vs["page_idx"], 0)], vs["page_idx"])
    assert out["set100"].tobytes() == vs.tobytes(), "set verdicts differ from the standalone matcher's"
    print("repeat %d: %s" % (r, {k: v[-1] for k, v in fps.items()}), flush=True)
m.use_page_set(0)
m.release_page_set(sid)
med = {k: float(np.median(v)) for k, v in fps.items()}
rec = dict(tool="page_set_rate", deck_pages=a.pages, deck_rows=m.descriptor_count, deck_unique_rows=m.unique_descriptor_count,
           frames=n, frame=[FW, FH], build_ms=build, fps=fps, fps_median=med,
           set_vs_standalone=round(med["set100"] / med["standalone100"] - 1.0, 4), set_vs_deck=round(med["set100"] / med["deck"], 2),
           verdicts_equal=True)
m.close(); sub.close()
print(json.dumps(rec))
