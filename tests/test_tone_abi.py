"""Match tone table (include/slideo_amd.h "Match tone table") without a GPU: the header, the exports and the mirrors; the pure host
function slideo_tone_lut against tests/tone_ref.py; the kernel's per-frame body compiled for the host (tools/tone_hostcheck.cpp) —
with and without -fsanitize=address,undefined — against the restatement on the constructed cases of the GPU test, the traces coming
from the CPU restatement of the pipeline (pyoracle); and the use on the darkened canvas scene through that restatement."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import evidence_ref as E
import levels_ref as LR
import tone_ref as T
import verify_cases as VC
from conftest import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["slideo_matcher_tone_begin", "slideo_matcher_tone_end", "slideo_matcher_tone_info", "slideo_matcher_tone_counts",
         "slideo_group_tone_begin", "slideo_group_tone_end", "slideo_group_tone_info", "slideo_group_tone_counts", "slideo_tone_lut"]


def test_exports_header_and_mirrors(capi):
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Match tone table" in header and "NOT the verdict" in header
    assert "#define SLIDEO_ABI_VERSION 7" in header
    for n in NAMES:
        assert n + "(" in header
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    for n in NAMES:
        assert "pub fn %s(" % n in ffi
    for n in ("tone_begin", "tone_end", "tone_info", "tone_counts"):
        assert n in hpp and hasattr(capi.Matcher, n) and hasattr(capi.Group, n)
    assert "tone_lut" in hpp and callable(capi.tone_lut)
    from slideo_amd import matching
    import inspect
    sig = inspect.signature(matching.learn_frame_levels_from_matches)
    for n in ("min_inliers", "min_hits", "min_count"):           # keyword-only, and none has a default: they depend on the content
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is inspect.Parameter.empty
    assert sig.parameters["flat"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["flat"].default == 255
    for doc in ("README.md", os.path.join("docs", "EXTENSIONS.md")):
        assert "Match tone table" in open(os.path.join(ROOT, doc)).read(), doc
    # the kernel header is compiled by stage_verify alone, and a change to it rebuilds that unit
    from slideo_amd import build
    assert "tone.hip.h" in build.HIP_UNIT_HEADERS["stage_verify.hip"]


def test_null_handle_refusals(capi):
    """Every entry point refuses a null handle with SLIDEO_ERR_INVALID_ARG and touches nothing it was given."""
    L = capi.lib()
    i32, i64 = [C.c_int32(7) for _ in range(3)], [C.c_int64(7) for _ in range(2)]
    buf = np.full((2, 3, 256), 7, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for pre in ("slideo_matcher_", "slideo_group_"):
        assert getattr(L, pre + "tone_begin")(None, 0, 1, 255) == 1
        assert getattr(L, pre + "tone_end")(None) == 1
        assert getattr(L, pre + "tone_info")(None, C.byref(i32[0]), C.byref(i32[1]), C.byref(i32[2]), C.byref(i64[0])) == 1
        assert getattr(L, pre + "tone_counts")(None, p(buf[0]), p(buf[1]), C.byref(i64[0]), C.byref(i64[1])) == 1
    assert all(v.value == 7 for v in i32 + i64) and (buf == 7).all()


def _arrays(rows):
    """cnt, sum uint64 [3, 256] with the same {value: (cnt, sum)} in every channel."""
    cnt, sm = np.zeros((3, 256), np.uint64), np.zeros((3, 256), np.uint64)
    for v, (n, s) in rows.items():
        cnt[:, v] = n; sm[:, v] = s
    return cnt, sm


def test_tone_lut_named_answers(capi):
    # one anchor: a constant table
    cnt, sm = _arrays({100: (10, 1234)})                       # mean (2468 + 10) // 20 = 123
    assert (capi.tone_lut(cnt, sm, 1) == 123).all()
    # anchors at 0 and 255: the straight line between their means, rounded half up
    cnt, sm = _arrays({0: (4, 40), 255: (2, 500)})             # 10 and 250
    lut = capi.tone_lut(cnt, sm, 1)
    assert lut[0, 0] == 10 and lut[0, 255] == 250
    assert lut[1, 17] == (2 * (10 * (255 - 17) + 250 * 17) + 255) // 510 == 26
    # a decreasing mean: the running maximum holds the table level
    cnt, sm = _arrays({10: (1, 50), 20: (1, 40), 30: (1, 90)})
    lut = capi.tone_lut(cnt, sm, 1)
    assert (lut[2, :21] == 50).all() and lut[2, 25] == 70 and (lut[2, 30:] == 90).all()
    # min_count: an anchor needs that many samples
    cnt, sm = _arrays({10: (5, 50), 20: (64, 64 * 200), 30: (63, 63 * 90)})
    assert (capi.tone_lut(cnt, sm, 64) == 200).all()
    with pytest.raises(capi.SlideoError) as e:                 # min_count excludes everything
        capi.tone_lut(cnt, sm, 65)
    assert e.value.code == 1
    # ties in the rounding: a mean of exactly x.5 goes up, an interpolated value of exactly x.5 goes up
    cnt, sm = _arrays({0: (2, 1), 2: (2, 5)})                  # means 0.5 -> 1 and 2.5 -> 3; lut[1] = (1 + 3) / 2 = 2
    lut = capi.tone_lut(cnt, sm, 1)
    assert list(lut[0, :3]) == [1, 2, 3]
    cnt, sm = _arrays({0: (1, 0), 2: (1, 1)})                  # lut[1] = 0.5 -> 1
    assert list(capi.tone_lut(cnt, sm, 1)[0, :3]) == [0, 1, 1]
    # one channel without an anchor refuses the whole table
    cnt, sm = _arrays({5: (3, 30)})
    cnt[1] = 0; sm[1] = 0
    with pytest.raises(capi.SlideoError):
        capi.tone_lut(cnt, sm, 1)


def test_tone_lut_equals_the_restatement_on_random_arrays(capi):
    rng = np.random.default_rng(29)
    n = 0
    for trial in range(60):
        dense = rng.uniform(0.01, 1.0)
        cnt = (rng.integers(0, 2 ** int(rng.integers(1, 40)), (3, 256), dtype=np.uint64) * (rng.uniform(0, 1, (3, 256)) < dense)).astype(np.uint64)
        sm = np.array([[int(rng.integers(0, 255 * int(c) + 1)) for c in row] for row in cnt], np.uint64)
        for min_count in (1, 2, 64, 2 ** 20):
            want = T.lut(cnt, sm, min_count)
            if want is None:
                with pytest.raises(capi.SlideoError):
                    capi.tone_lut(cnt, sm, min_count)
            else:
                got = capi.tone_lut(cnt, sm, min_count)
                assert np.array_equal(got, want), (trial, min_count)
                assert (np.diff(got.astype(int), axis=1) >= 0).all()          # monotone
                n += 1
    assert n > 100


def test_tone_lut_refusals(capi):
    """Each refusal returns SLIDEO_ERR_INVALID_ARG and leaves lut_out as it was."""
    L = capi.lib()
    cnt, sm = _arrays({5: (3, 30), 200: (4, 900)})
    out = np.full((3, 256), 7, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda c=cnt, s=sm, mc=1, o=out: L.slideo_tone_lut(p(c) if c is not None else None, p(s) if s is not None else None, C.c_int64(mc),
                                                               p(o) if o is not None else None)
    big, over = cnt.copy(), sm.copy()
    big[0, 5] = 2 ** 48 + 1
    over[2, 5] = 255 * 3 + 1                                    # a sum no session gives: a mean above 255
    for kw in (dict(c=None), dict(s=None), dict(o=None), dict(mc=0), dict(mc=-3), dict(mc=5), dict(c=big), dict(s=over)):
        assert call(**kw) == 1, kw
    assert (out == 7).all()
    assert call() == 0 and out[0, 0] == 10 and out[0, 255] == 225
    with pytest.raises(ValueError):
        capi.tone_lut(cnt[:2], sm, 1)


# ---- tools/tone_hostcheck.cpp ------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "tone_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tone"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tone_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


_traces = {}


def _oracle_unit(oracle, name, fa, pset):
    """A constructed case through the CPU restatement of the pipeline: (cfg, frames of tone_ref.counts, train_page, page_xy, pages).
    A page set is a deck of the selected pages alone; its page indices and train rows are mapped back to the whole deck's."""
    key = (name.split("-")[0] if name.startswith("T2") else name)
    if key in _traces:
        return _traces[key]
    case = VC.build(*fa)
    cfg = small_cfg(oracle, **case.cfg)
    train, tp, pxy = case.deck()
    sel = list(range(len(case.pages))) if pset is None else sorted(pset)
    db = oracle.PageDB(cfg)
    pages = {}
    for i in sel:
        pg = case.pages[i]
        w, h = T.page_size(case, i)
        small = oracle.small_image(T.page_pixels(case, i), cfg.small_area)
        pages[i] = (w, h, small)
        db.add_page_features(w, h, VC.keypoints(pg.xy), pg.desc, small)
    assert db.finalize() == 0
    rows = None if pset is None else np.nonzero(np.isin(tp, sel))[0]
    frames = []
    for fi, f in enumerate(case.frames):
        v, cands = db.match_features_trace(case.frame_pixels(fi), VC.keypoints(f.xy), f.desc)
        cands = [{"page_idx": sel[int(c["page_idx"])], "transform": c["transform"], "n_votes": int(c["n_votes"]), "inliers": int(c["inliers"])}
                 for c in cands]
        rec = T.frame_record(cfg, f.xy, f.desc, cands, train, case.frame_pixels(fi), rows)
        rec["order"] = [(c["page_idx"], c["n_votes"]) for c in cands]
        rec["verdict"] = sel[int(v["page_idx"])] if v["page_idx"] >= 0 else -1
        frames.append(rec)
    _traces[key] = (cfg, frames, tp, pxy, pages)
    return _traces[key]


def _write_unit(path, cfg, frames, tp, pxy, pages, min_inliers, min_hits, flat, flags=0, rerun_mask=12):
    """The unit as the device holds it: the votes of a frame at qofs[f] * k, a candidate's run at its ofs, in candidate order; the
    pages' records and small images (a page that is not in the deck: a 1 x 1 image nobody reads)."""
    k = cfg.knn_k
    qofs = np.concatenate([[0], np.cumsum([len(f["xy"]) for f in frames])]).astype(np.uint32)
    qtot = int(qofs[-1])
    votes = np.zeros((qtot * k, 2), np.uint32)
    tail = b""
    for fi, f in enumerate(frames):
        at = 0
        tail += struct.pack("<i", len(f["order"]))
        for (page, n_votes), (_, inliers, M) in zip(f["order"], f["cands"]):
            run = [(q, t) for q, t in f["votes"] if tp[t] == page]
            assert len(run) == n_votes, "the votes of evidence_ref.votes_of are not the trace's"
            base = int(qofs[fi]) * k + at
            votes[base:base + len(run)] = np.array(run, np.uint32).reshape(-1, 2)
            M = np.asarray(M, np.float64)
            tail += struct.pack("<5i", page, len(run), at, inliers, int(np.any(M != 0))) + M.tobytes()
            at += len(run)
    kp = np.concatenate([VC.keypoints(f["xy"]) for f in frames]) if qtot else np.zeros(0, VC.KEYPOINT_DTYPE)
    ah, aw = frames[0]["image"].shape[:2]
    npages = int(tp.max()) + 1
    with open(path, "wb") as o:
        o.write(struct.pack("<16i", cfg.verify_model, k, aw, ah, min_inliers, min_hits, flat, len(frames), len(tp), qtot, flags, rerun_mask, npages, 0, 0, 0))
        o.write(struct.pack("<d", cfg.ransac_threshold))
        o.write(qofs.tobytes()); o.write(kp.tobytes())
        o.write(np.ascontiguousarray(pxy, np.float32).tobytes()); o.write(votes.tobytes()); o.write(tail)
        smalls = []
        for p in range(npages):
            w, h, small = pages.get(p, (1, 1, np.zeros((1, 1, 3), np.uint8)))
            o.write(struct.pack("<4i", w, h, small.shape[1], small.shape[0]))
            smalls.append(np.ascontiguousarray(small, np.uint8).tobytes())
        o.write(b"".join(smalls))
        for f in frames:
            o.write(np.ascontiguousarray(f["image"], np.uint8).tobytes())


def _host_counts(exe, tmp, unit_args, tile_rows=None):
    unit, out = str(tmp / "unit.bin"), str(tmp / "out.bin")
    _write_unit(unit, *unit_args)
    stats = subprocess.check_output([exe, unit, out] + ([str(tile_rows)] if tile_rows else [])).decode().split()
    got = np.fromfile(out, np.uint64)
    assert got.size == 1537
    return got[:768].reshape(3, 256), got[768:1536].reshape(3, 256), int(got[1536]), dict(zip(stats[::2], map(int, stats[1::2])))


def _check_cases(oracle, exe, tmp):
    seen = set()
    for name, fa, pset, min_inliers, min_hits, flats in T.constructed_cases():
        cfg, frames, tp, pxy, pages = _oracle_unit(oracle, name, fa, pset)
        for flat in flats:
            stats = []
            want = T.counts(frames, min_inliers=min_inliers, min_hits=min_hits, flat=flat, model=cfg.verify_model, thr=cfg.ransac_threshold,
                            train_page=tp, page_xy=pxy, pages=pages, stats=stats)          # (asserts the guard on every tested value)
            cnt, sm, counted, hs = _host_counts(exe, tmp, (cfg, frames, tp, pxy, pages, min_inliers, min_hits, flat))
            assert np.array_equal(cnt, want[0]) and np.array_equal(sm, want[1]) and counted == want[3], (name, flat)
            assert hs["hits"] == sum(s[2] for s in stats if s) and hs["tiles"] <= 1
            # the same through row tiles of 7 rows: the tile seam
            cnt7, sm7, counted7, hs7 = _host_counts(exe, tmp, (cfg, frames, tp, pxy, pages, min_inliers, min_hits, flat), tile_rows=7)
            assert np.array_equal(cnt7, cnt) and np.array_equal(sm7, sm) and counted7 == counted and (counted == 0 or hs7["tiles"] > 10)
            _statements(name, frames, pages, stats, want, flat, seen)
    assert seen >= {"other-page", "no-verdict", "outside", "two-sizes", "flat-thins", "empty-frame", "model1", "set"}
    # a unit whose run raised a re-run bit counts nothing
    name, fa, pset, mi, mh, flats = T.constructed_cases()[0]
    cfg, frames, tp, pxy, pages = _oracle_unit(oracle, name, fa, pset)
    for flags, mask, counts in ((4, 12, False), (8, 12, False), (8, 4, True), (2, 12, True)):
        cnt, sm, counted, _ = _host_counts(exe, tmp, (cfg, frames, tp, pxy, pages, mi, mh, 255, flags, mask))
        assert bool(cnt.sum()) == counts and bool(counted) == counts, (flags, mask)


_flat_samples = {}


def _statements(name, frames, pages, stats, want, flat, seen):
    """What each constructed case is there for, stated on the restatement's own figures."""
    if name in ("T2-inliers", "T2-hits"):
        assert want[3] == 0 and int(want[0].sum()) == 0 and T.contributor(frames[0]["cands"], 0) >= 0, name
        return
    assert want[3] >= 1 and (int(want[0].sum()) > 0 or flat < 2), name      # (flat 0 on a smooth gradient: every pixel has a differing neighbour)
    for f, s in zip(frames, stats):
        if s is None:
            continue
        n, (bx0, by0, bx1, by1), hits, page = s
        w, h, small = pages[page]
        assert 0 < bx0 and 0 < by0 and bx1 < w - 1 and by1 < h - 1, (name, "the hit box clips the page")
        if f["verdict"] >= 0 and f["verdict"] != page:
            seen.add("other-page")
        if f["verdict"] < 0:
            seen.add("no-verdict")
        if (w, h) != (VC.PAGE_W, VC.PAGE_H):
            seen.add("two-sizes")
    if name == "OUT" and flat == 255:
        # every small pixel inside the box is a sample unless its image leaves the frame
        n, (bx0, by0, bx1, by1), hits, page = stats[0]
        w, h, small = pages[page]
        sh, sw = small.shape[:2]
        x = ((np.arange(sw) + 0.5) * w) / sw - 0.5; y = ((np.arange(sh) + 0.5) * h) / sh - 0.5
        inside = int(((x >= bx0) & (x <= bx1)).sum()) * int(((y >= by0) & (y <= by1)).sum())
        assert 0 < n < 0.95 * inside, (n, inside)
        seen.add("outside")
    if name == "D2-other":
        _flat_samples[flat] = int(want[0][0].sum())
        if len(_flat_samples) == 4:
            assert _flat_samples[0] < _flat_samples[2] < _flat_samples[8] < _flat_samples[255], _flat_samples
            seen.add("flat-thins")
    if name == "V1-empty":
        assert any(len(f["xy"]) == 0 for f in frames) and want[3] == sum(1 for f in frames if len(f["xy"]) > 1)
        seen.add("empty-frame")
    if name == "H1":
        seen.add("model1")
    if name == "V5-set":
        seen.add("set")


def test_host_build_of_the_kernel_body_equals_the_restatement(oracle, hostcheck, tmp_path):
    _flat_samples.clear()
    _check_cases(oracle, hostcheck, tmp_path)


def test_sanitized_host_build_over_the_constructed_cases(oracle, hostcheck_san, tmp_path):
    """Address and undefined-behaviour checks with every array in an allocation of exactly its size.  A stand-alone program: nothing
    is loaded into Python."""
    _flat_samples.clear()
    _check_cases(oracle, hostcheck_san, tmp_path)


def test_wild_features_reach_no_counter(oracle, hostcheck_san, tmp_path):
    """A caller's own features may hold any float: keypoints and a transform that send samples to negative, huge, infinite or NaN
    positions count nowhere and read nothing outside the frame (the sanitized build)."""
    name, fa, pset, mi, mh, flats = T.constructed_cases()[0]
    cfg, frames, tp, pxy, pages = _oracle_unit(oracle, name, fa, pset)
    slot = T.contributor(frames[0]["cands"], 0)
    for k, wild in enumerate(([1e300, 0, 0, 0, 1e300, 0], [np.nan] * 6, [np.inf, 0, 5, 0, -np.inf, 5], [1, 0, -1e9, 0, 1, 2.0 ** 40], [0, 0, 639.4, 0, 0, 359.4])):
        f = dict(frames[0])
        f["cands"] = list(f["cands"])
        M = np.array(f["cands"][slot][2], np.float64, copy=True)
        M[:6] = wild
        f["cands"][slot] = (f["cands"][slot][0], f["cands"][slot][1], M)
        # (no vote passes under such a transform: min_hits 1 would end the frame, so the test is of tone_votes; the last one maps
        # every page point to the frame's last pixel and no keypoint sits there either)
        want = T.counts([f], min_inliers=mi, min_hits=1, flat=255, model=cfg.verify_model, thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy,
                        pages=pages, guard=False)
        cnt, sm, counted, _ = _host_counts(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, pages, mi, 1, 255))
        assert np.array_equal(cnt, want[0]) and np.array_equal(sm, want[1]) and counted == want[3], k
    # keypoints moved wildly under the true transform: the hits are the untouched ones, and the samples stay inside the frame
    f = dict(frames[0]); f["xy"] = np.array(f["xy"], np.float32, copy=True)
    f["xy"][:6] = [[-0.5, 10], [10, -3e9], [1e30, 10], [10, 360], [np.nan, 10], [np.inf, -np.inf]]
    want = T.counts([f], min_inliers=mi, min_hits=1, flat=255, model=cfg.verify_model, thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy, pages=pages,
                    guard=False)
    cnt, sm, counted, _ = _host_counts(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, pages, mi, 1, 255))
    assert np.array_equal(cnt, want[0]) and np.array_equal(sm, want[1]) and counted == want[3] == 1


# ---- the use -------------------------------------------------------------------------------------------------------------------------

def test_the_use_scene_meets_its_conditions_on_the_cpu(capi, oracle, synth):
    """The canvas scene of the evidence map (tests/evidence_ref.py canvas_scene: a 640x360 window in a 960x540 textured canvas, 4 pages,
    16 frames, ORB-3000, min_rating 12) with the window alone darkened as a projector would (tone_ref.darken), through the CPU
    restatement of the pipeline, evidence_ref.votes_of and tone_ref, at min_inliers 20, min_hits 20, flat 255, min_count 64:
      - the darkened frames give at least 3 of 16 verdicts that are not the truth;
      - the table learnt from them gives the truth on all 16 with every similarity at least 0.70;
      - the table learnt from the clean frames changes no verdict of the clean frames;
      - at least 10 frames contribute.
    The library's slideo_tone_lut gives the restatement's table on these counts.
    Found, not gated: the blind stretch of the levels histogram (1 % cut at either end) has the points lo (14, 14, 14), hi (254, 254,
    253) on these frames — the canvas's tones, nearly the identity — and gets 14 of 16 pages right; 4 of the 16 darkened frames are
    wrong without a table; 13 frames contribute 610 808 samples, and the lowest similarity under the learnt table is 0.760."""
    pages, frames, truth = E.canvas_scene(synth)
    U = T.USE
    cfg = small_cfg(oracle, nfeatures=E.SCENE["nfeatures"], min_rating=U["min_rating"])
    db = oracle.PageDB(cfg)
    db.add_pages(pages, threads=4)
    assert db.finalize() == 0
    train = db.train()
    tp, pxy = E.deck_of(db, len(pages))
    page_recs = {p: (pages[p].shape[1], pages[p].shape[0], oracle.small_image(pages[p], cfg.small_area)) for p in range(len(pages))}

    def learn(fr):
        recs = []
        for f in fr:
            _, cands = db.match_frame_trace(f)
            kp, desc = oracle.orb(f, cfg)
            recs.append(T.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, cands, train, f))
        cnt, sm, through, counted = T.counts(recs, min_inliers=U["min_inliers"], min_hits=U["min_hits"], flat=U["flat"], model=0,
                                             thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy, pages=page_recs, guard=False)
        return cnt, sm, counted

    dark = T.darken(frames)
    vd = db.match_frames(dark, threads=8)
    wrong = int((vd["page_idx"] != truth).sum())
    cnt, sm, counted = learn(dark)
    lut = T.lut(cnt, sm, U["min_count"])
    assert lut is not None and np.array_equal(capi.tone_lut(cnt, sm, U["min_count"]), lut)
    vl = db.match_frames(LR.apply(dark, lut), threads=8)
    lo, hi = LR.points(LR.histogram(dark), 10000, 10000)
    vb = db.match_frames(LR.apply(dark, LR.stretch_lut(lo, hi)), threads=8)
    print("the use on the CPU: %d of 16 wrong when darkened; %d frames contributed, %d samples; learnt table: %d right, lowest similarity %.3f; "
          "blind stretch: points %s %s, %d right" % (wrong, counted, int(cnt[0].sum()), int((vl["page_idx"] == truth).sum()),
                                                     float(vl["similarity"].min()), lo, hi, int((vb["page_idx"] == truth).sum())))
    assert wrong >= 3
    assert counted >= 10
    assert (vl["page_idx"] == truth).all() and float(vl["similarity"].min()) >= 0.70
    ccnt, csm, ccounted = learn(frames)
    clut = T.lut(ccnt, csm, U["min_count"])
    v0 = db.match_frames(frames, threads=8)
    v1 = db.match_frames(LR.apply(frames, clut), threads=8)
    assert np.array_equal(v0["page_idx"], v1["page_idx"]) and (v0["page_idx"] == truth).all()
