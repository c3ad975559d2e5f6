"""Match evidence map (include/slideo_amd.h "Match evidence map") without a GPU: the header, the exports and the mirrors; the two
pure host functions against tests/evidence_ref.py on random count arrays; and the kernel's per-frame body compiled for the host
(tools/evidence_hostcheck.cpp) — with and without -fsanitize=address,undefined — against the restatement on the constructed cases of
the GPU test, the traces coming from the CPU restatement of the pipeline (pyoracle)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import evidence_ref as E
import verify_cases as VC
from conftest import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["slideo_matcher_evidence_begin", "slideo_matcher_evidence_end", "slideo_matcher_evidence_info", "slideo_matcher_evidence_counts",
         "slideo_group_evidence_begin", "slideo_group_evidence_end", "slideo_group_evidence_info", "slideo_group_evidence_counts",
         "slideo_evidence_mask", "slideo_evidence_box"]


def test_exports_header_and_mirrors(capi):
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Match evidence map" in header and "NOT RANSAC's inlier mask" in header
    assert "#define SLIDEO_ABI_VERSION 7" in header
    for n in NAMES:
        assert n + "(" in header
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    for n in NAMES:
        assert "pub fn %s(" % n in ffi
    for n in ("evidence_begin", "evidence_end", "evidence_info", "evidence_counts"):
        assert n in hpp and hasattr(capi.Matcher, n) and hasattr(capi.Group, n)
    from slideo_amd import matching
    import inspect
    for fn, names in ((matching.learn_frame_mask_from_matches, ("cell", "min_inliers", "min_seen", "min_hit", "grow")),
                      (matching.learn_frame_box_from_matches, ("cell", "min_inliers", "min_hits", "min_hit"))):
        sig = inspect.signature(fn)
        for n in names:                                   # keyword-only, and none has a default: they depend on the content
            assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is inspect.Parameter.empty
    sig = inspect.signature(matching.learn_frame_box_from_matches)
    assert sig.parameters["inset"].default == 0 and sig.parameters["out_size"].default is None
    for doc in ("README.md", os.path.join("docs", "EXTENSIONS.md")):
        assert "Match evidence map" in open(os.path.join(ROOT, doc)).read(), doc


SIZES = ((402, 300), (403, 33), (640, 360), (64, 64), (1, 1))


def _random_counts(rng, aw, ah, cell, kind):
    gw, gh = E.grid(aw, ah, cell)
    if kind == "zero":
        return np.zeros((gh, gw), np.uint32), np.zeros((gh, gw), np.uint32)
    seen = rng.integers(0, 40, (gh, gw)).astype(np.uint32)
    if kind == "big":
        seen = rng.integers(0, 2 ** 32, (gh, gw), dtype=np.uint64).astype(np.uint32)
    hit = (seen * rng.uniform(0, 1, (gh, gw))).astype(np.uint32)
    if kind == "clutter":
        hit[:] = 0; seen[:] = np.maximum(seen, 1)
    return seen, hit


def test_mask_and_box_equal_the_restatement(capi):
    rng = np.random.default_rng(5)
    n = 0
    for aw, ah in SIZES:
        for cell in (16, 32, 64):
            for kind in ("random", "zero", "big", "clutter"):
                seen, hit = _random_counts(rng, aw, ah, cell, kind)
                for grow in (0, 1, 3):
                    for ppm in (0, 1, 250000, 1000000):
                        for min_seen in (0, 5):
                            got = capi.evidence_mask(seen, hit, cell, aw, ah, min_seen, ppm / 1e6, grow)
                            want = E.mask(seen, hit, cell, aw, ah, min_seen, ppm, grow)
                            assert got.shape == (ah, aw) and np.array_equal(got, want), (aw, ah, cell, kind, grow, ppm, min_seen)
                            n += 1
                for ppm in (0, 1, 250000, 1000000):
                    for min_hits in (0, 1, 7, 2 ** 32 - 1):
                        assert capi.evidence_box(seen, hit, cell, aw, ah, min_hits, ppm / 1e6) == E.box(seen, hit, cell, aw, ah, min_hits, ppm), \
                            (aw, ah, cell, kind, ppm, min_hits)
    assert n > 1000


def test_mask_and_box_named_answers(capi):
    """All clutter: every cell has keypoints and none agrees — the mask is all zero, the box all -1.  No cell with a keypoint: the mask
    keeps everything (nothing is known), and a box that asks for one hit finds none.  grow reaches across the whole grid."""
    aw, ah, cell = 402, 300, 32
    gw, gh = E.grid(aw, ah, cell)
    seen, hit = np.full((gh, gw), 9, np.uint32), np.zeros((gh, gw), np.uint32)
    assert not capi.evidence_mask(seen, hit, cell, aw, ah, 1, 0.5, 3).any()
    assert capi.evidence_box(seen, hit, cell, aw, ah, 1, 0.0) == (-1, -1, -1, -1)
    zero = np.zeros((gh, gw), np.uint32)
    assert (capi.evidence_mask(zero, zero, cell, aw, ah, 1, 1.0, 0) == 255).all()
    assert capi.evidence_box(zero, zero, cell, aw, ah, 1, 0.0) == (-1, -1, -1, -1)
    assert capi.evidence_box(zero, zero, cell, aw, ah, 0, 0.0) == (0, 0, aw, ah)          # (every cell qualifies at 0 hits: the image)
    hit[3, 5] = 9
    m = capi.evidence_mask(seen, hit, cell, aw, ah, 1, 0.5, 1)
    assert (m[64:160, 128:224] == 255).all() and m.sum() == 255 * 96 * 96
    assert capi.evidence_box(seen, hit, cell, aw, ah, 9, 1.0) == (160, 96, 192, 128)
    hit[gh - 1, gw - 1] = 9                                                             # the last, partial cell: clipped to the image
    assert capi.evidence_box(seen, hit, cell, aw, ah, 9, 1.0) == (160, 96, aw, ah)
    assert (capi.evidence_mask(seen, hit, cell, aw, ah, 1, 0.5, 256) == 255).all()


def test_argument_refusals(capi):
    L = capi.lib()
    aw, ah, cell = 100, 50, 16
    gw, gh = E.grid(aw, ah, cell)
    seen = np.zeros((gh, gw), np.uint32); hit = seen.copy()
    out = np.zeros((ah, aw), np.uint8); box = (C.c_int32 * 4)(7, 7, 7, 7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def mask(seen_=p(seen), hit_=p(hit), gw_=gw, gh_=gh, cell_=cell, aw_=aw, ah_=ah, min_seen=1, ppm=10, grow=0, out_=p(out), stride=aw):
        return L.slideo_evidence_mask(seen_, hit_, gw_, gh_, cell_, aw_, ah_, C.c_int64(min_seen), ppm, grow, out_, C.c_int64(stride))

    def fbox(seen_=p(seen), hit_=p(hit), gw_=gw, gh_=gh, cell_=cell, aw_=aw, ah_=ah, min_hits=1, ppm=10, out_=box):
        return L.slideo_evidence_box(seen_, hit_, gw_, gh_, cell_, aw_, ah_, C.c_int64(min_hits), ppm, out_)

    assert mask() == 0 and fbox() == 0
    out[:] = 7
    for kw in (dict(seen_=None), dict(hit_=None), dict(out_=None), dict(cell_=8), dict(cell_=48), dict(cell_=128), dict(gw_=gw + 1), dict(gh_=gh - 1),
               dict(aw_=0), dict(ah_=0), dict(aw_=4097, gw_=257), dict(min_seen=-1), dict(min_seen=2 ** 32), dict(ppm=-1), dict(ppm=1000001),
               dict(grow=-1), dict(grow=257), dict(stride=aw - 1)):
        assert mask(**kw) == 1, kw
    assert (out == 7).all()                                 # a refused call writes nothing
    for kw in (dict(seen_=None), dict(hit_=None), dict(out_=None), dict(cell_=0), dict(gw_=gw - 1), dict(ah_=-5), dict(min_hits=-1),
               dict(min_hits=2 ** 32), dict(ppm=-1), dict(ppm=1000001)):
        assert fbox(**kw) == 1, kw
    assert mask(stride=aw + 3, out_=p(np.zeros((ah, aw + 3), np.uint8))) == 0
    with pytest.raises(capi.SlideoError):
        capi.evidence_mask(seen, hit, 24, aw, ah, 1, 0.5, 0)
    with pytest.raises(ValueError):
        capi.evidence_box(seen, hit[:1], cell, aw, ah, 1, 0.5)


# ---- tools/evidence_hostcheck.cpp ----------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "evidence_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("evidence"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("evidence_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


_traces = {}


def _oracle_unit(oracle, name, fa, pset):
    """A constructed case through the CPU restatement of the pipeline: (cfg, frames of evidence_ref.counts, train_page, page_xy).  A
    page set is a deck of the selected pages alone; its page indices and train rows are mapped back to the whole deck's."""
    if name in _traces:
        return _traces[name]
    case = VC.build(*fa)
    cfg = small_cfg(oracle, **case.cfg)
    train, tp, pxy = case.deck()
    sel = list(range(len(case.pages))) if pset is None else sorted(pset)
    db = oracle.PageDB(cfg)
    smalls = {}
    for i in sel:
        pg = case.pages[i]
        if pg.img not in smalls:
            smalls[pg.img] = oracle.small_image(VC.page_image(pg.img), cfg.small_area)
        db.add_page_features(VC.PAGE_W, VC.PAGE_H, VC.keypoints(pg.xy), pg.desc, smalls[pg.img])
    assert db.finalize() == 0
    rows = None if pset is None else np.nonzero(np.isin(tp, sel))[0]
    frames = []
    for fi, f in enumerate(case.frames):
        v, cands = db.match_features_trace(case.frame_pixels(fi), VC.keypoints(f.xy), f.desc)
        v = {"page_idx": sel[int(v["page_idx"])] if v["page_idx"] >= 0 else -1, "inliers": int(v["inliers"])}
        cands = [{"page_idx": sel[int(c["page_idx"])], "transform": c["transform"], "n_votes": int(c["n_votes"])} for c in cands]
        rec = E.frame_record(cfg, f.xy, f.desc, v, cands, train, rows)
        rec["order"] = [(c["page_idx"], c["n_votes"]) for c in cands]
        frames.append(rec)
    _traces[name] = (cfg, frames, tp, pxy)
    return _traces[name]


def _write_unit(path, cfg, frames, tp, pxy, cell, aw, ah, min_inliers, flags=0, rerun_mask=12):
    """The unit as the device holds it: the votes of a frame at qofs[f] * k, a candidate's run at its ofs, in candidate order."""
    k = cfg.knn_k
    qofs = np.concatenate([[0], np.cumsum([len(f["xy"]) for f in frames])]).astype(np.uint32)
    qtot = int(qofs[-1])
    votes = np.zeros((qtot * k, 2), np.uint32)
    tail = b""
    for fi, f in enumerate(frames):
        at = 0
        tail += struct.pack("<i", len(f["order"]))
        for page, n_votes in f["order"]:
            run = [(q, t) for q, t in f["votes"] if tp[t] == page]
            assert len(run) == n_votes, "the votes of evidence_ref.votes_of are not the trace's"
            base = int(qofs[fi]) * k + at
            votes[base:base + len(run)] = np.array(run, np.uint32).reshape(-1, 2)
            tail += struct.pack("<3i", page, len(run), at) + np.asarray(f["cands"][page], np.float64).tobytes()
            at += len(run)
    kp = np.concatenate([VC.keypoints(f["xy"]) for f in frames]) if qtot else np.zeros(0, VC.KEYPOINT_DTYPE)
    verdicts = np.array([[f["page"], 0, f["inliers"], len(f["xy"])] for f in frames], np.int32)
    with open(path, "wb") as o:
        o.write(struct.pack("<12i", cfg.verify_model, k, cell, aw, ah, min_inliers, len(frames), len(tp), qtot, flags, rerun_mask, 0))
        o.write(struct.pack("<d", cfg.ransac_threshold))
        o.write(qofs.tobytes()); o.write(verdicts.tobytes()); o.write(kp.tobytes())
        o.write(np.ascontiguousarray(pxy, np.float32).tobytes()); o.write(votes.tobytes()); o.write(tail)


def _host_counts(exe, tmp, unit_args, cell, aw, ah):
    unit, out = str(tmp / "unit.bin"), str(tmp / "out.bin")
    _write_unit(unit, *unit_args)
    stats = subprocess.check_output([exe, unit, out]).decode().split()
    got = np.fromfile(out, np.uint32)
    gw, gh = E.grid(aw, ah, cell)
    assert got.size == 2 * gw * gh
    return got[:gw * gh].reshape(gh, gw), got[gw * gh:].reshape(gh, gw), dict(zip(stats[::2], map(int, stats[1::2])))


def _check_cases(oracle, exe, tmp):
    most_windows = counted_frames = hits = below = 0
    for name, fa, pset, min_inliers in E.constructed_cases():
        cfg, frames, tp, pxy = _oracle_unit(oracle, name, fa, pset)
        for cell in (16, 32, 64):
            want = E.counts(frames, cell=cell, aw=VC.FRAME_W, ah=VC.FRAME_H, min_inliers=min_inliers, model=cfg.verify_model,
                            thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy)          # (asserts the guard on every tested pair)
            seen, hit, stats = _host_counts(exe, tmp, (cfg, frames, tp, pxy, cell, VC.FRAME_W, VC.FRAME_H, min_inliers), cell, VC.FRAME_W, VC.FRAME_H)
            assert np.array_equal(seen, want[0]) and np.array_equal(hit, want[1]), (name, cell)
            most_windows = max(most_windows, stats["windows"])
        counted_frames += want[3]; hits += int(want[1].sum())
        below += sum(1 for f in frames if f["page"] >= 0 and f["inliers"] < min_inliers)
        if name == "MULTI":                 # every keypoint has two votes for the winner, of which exactly one passes
            f = frames[0]
            assert f["page"] == 0 and len(f["votes"]) == 2 * len(f["xy"]) and int(want[1].sum()) == len(f["xy"])
        if name in ("X1-none", "T2-below"):
            assert want[3] == 0 and int(want[0].sum()) == 0, name
    assert most_windows >= 2 and counted_frames > 5 and hits > 1000 and below >= 1
    # a unit whose run raised a re-run bit counts nothing
    name, fa, pset, mi = E.constructed_cases()[0]
    cfg, frames, tp, pxy = _oracle_unit(oracle, name, fa, pset)
    for flags, mask, counts in ((4, 12, False), (8, 12, False), (8, 4, True), (2, 12, True)):
        seen, hit, _ = _host_counts(exe, tmp, (cfg, frames, tp, pxy, 32, VC.FRAME_W, VC.FRAME_H, mi, flags, mask), 32, VC.FRAME_W, VC.FRAME_H)
        assert bool(seen.sum()) == counts, (flags, mask)


def test_host_build_of_the_kernel_body_equals_the_restatement(oracle, hostcheck, tmp_path):
    _check_cases(oracle, hostcheck, tmp_path)


def test_sanitized_host_build_over_the_constructed_cases(oracle, hostcheck_san, tmp_path):
    """Address and undefined-behaviour checks with every array in an allocation of exactly its size.  A stand-alone program: nothing
    is loaded into Python."""
    _check_cases(oracle, hostcheck_san, tmp_path)


def test_keypoints_outside_the_image_have_no_cell(oracle, hostcheck_san, tmp_path):
    """A caller's own features may hold any float: a keypoint at a negative, too large, infinite or NaN position counts nowhere and
    reaches no counter (the sanitized build)."""
    name, fa, pset, mi = E.constructed_cases()[1]
    cfg, frames, tp, pxy = _oracle_unit(oracle, name, fa, pset)
    f = dict(frames[0]); f["xy"] = np.array(f["xy"], np.float32, copy=True)
    n = len(f["xy"])
    f["xy"][:6] = [[-0.5, 10], [10, -3], [640, 10], [10, 360], [np.nan, 10], [np.inf, -np.inf]]
    want = E.counts([f], cell=16, aw=VC.FRAME_W, ah=VC.FRAME_H, min_inliers=mi, model=cfg.verify_model, thr=cfg.ransac_threshold,
                    train_page=tp, page_xy=pxy, guard=False)
    seen, hit, _ = _host_counts(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, 16, VC.FRAME_W, VC.FRAME_H, mi), 16, VC.FRAME_W, VC.FRAME_H)
    assert np.array_equal(seen, want[0]) and np.array_equal(hit, want[1]) and int(seen.sum()) == n - 6


def test_the_use_scene_meets_its_conditions_on_the_cpu(capi, oracle, synth):
    """The scene of the GPU test "the use" through the CPU restatement of the pipeline (ORB, match, trace) and evidence_ref: the box
    and mask conditions hold on it without the library's kernels; the library's two host functions give the restatement's box and
    mask on these counts.  (The restatement has no frame mask: the inliers condition is the GPU test's.)"""
    pages, frames, truth = E.canvas_scene(synth)
    S = E.SCENE
    cfg = small_cfg(oracle, nfeatures=S["nfeatures"])
    db = oracle.PageDB(cfg)
    db.add_pages(pages, threads=4)
    assert db.finalize() == 0
    train = db.train()
    tp, pxy = E.deck_of(db, len(pages))
    recs = []
    for f in frames:
        v, cands = db.match_frame_trace(f)
        kp, desc = oracle.orb(f, cfg)
        recs.append(E.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, v, cands, train))
    assert np.mean([r["page"] == t for r, t in zip(recs, truth)]) >= 0.75
    seen, hit, through, counted = E.counts(recs, cell=S["cell"], aw=E.CANVAS_W, ah=E.CANVAS_H, min_inliers=S["min_inliers"], model=0,
                                           thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy)
    box = E.box(seen, hit, S["cell"], E.CANVAS_W, E.CANVAS_H, S["min_hits"], int(S["box_min_hit"] * 1e6))
    mask = E.mask(seen, hit, S["cell"], E.CANVAS_W, E.CANVAS_H, S["min_seen"], int(S["min_hit"] * 1e6), S["grow"])
    zeroed, outside = E.check_use(seen, hit, S["cell"], S["min_seen"], box, mask)
    print("the use on the CPU: %d of %d counted, box %s, %d of %d clutter cells zeroed" % (counted, through, box, zeroed, outside))
    assert capi.evidence_box(seen, hit, S["cell"], E.CANVAS_W, E.CANVAS_H, S["min_hits"], S["box_min_hit"]) == box
    assert np.array_equal(capi.evidence_mask(seen, hit, S["cell"], E.CANVAS_W, E.CANVAS_H, S["min_seen"], S["min_hit"], S["grow"]), mask)
