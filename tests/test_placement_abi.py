"""Match placement map (include/slideo_amd.h "Match placement map") without a GPU: the header, the exports and the mirrors; the pure host
function slideo_placement_quad against tests/placement_ref.py; the kernel's per-frame body compiled for the host
(tools/placement_hostcheck.cpp) — with and without -fsanitize=address,undefined — against the restatement on the constructed cases of
the GPU test, the traces coming from the CPU restatement of the pipeline (pyoracle); and the use on the keystone scene through that
restatement."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import evidence_ref as E
import placement_ref as P
import tone_ref as T
import verify_cases as VC
from conftest import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["slideo_matcher_placement_begin", "slideo_matcher_placement_end", "slideo_matcher_placement_info", "slideo_matcher_placement_sums",
         "slideo_group_placement_begin", "slideo_group_placement_end", "slideo_group_placement_info", "slideo_group_placement_sums",
         "slideo_placement_quad"]


def test_exports_header_and_mirrors(capi):
    L = capi.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Match placement map" in header and "NOT the verdict's winner" in header and "ESTIMATOR" in header
    assert "fixed camera and screen" in header and "2^52" in header and "SLIDEO_PLACEMENT_MAX_FRAMES" in header
    assert "which the traces' transforms can give on the host" not in header
    assert "#define SLIDEO_ABI_VERSION 7" in header
    for n in NAMES:
        assert n + "(" in header
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    for n in NAMES:
        assert "pub fn %s(" % n in ffi
    for n in ("placement_begin", "placement_end", "placement_info", "placement_sums"):
        assert n in hpp and hasattr(capi.Matcher, n) and hasattr(capi.Group, n)
    assert "placement_quad" in hpp and callable(capi.placement_quad)
    from slideo_amd import matching
    import inspect
    sig = inspect.signature(matching.learn_frame_quad_from_matches)
    for n in ("cell", "min_inliers", "reach", "min_count", "trim", "rounds"):      # keyword-only, and none has a default
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[n].default is inspect.Parameter.empty
    assert sig.parameters["inset"].default == 0 and sig.parameters["out_size"].default is None
    for doc in ("README.md", os.path.join("docs", "EXTENSIONS.md")):
        assert "Match placement map" in open(os.path.join(ROOT, doc)).read(), doc
    from slideo_amd import build
    assert "placement.hip.h" in build.HIP_UNIT_HEADERS["stage_verify.hip"]


def test_null_handle_refusals(capi):
    """Every entry point refuses a null handle with SLIDEO_ERR_INVALID_ARG and touches nothing it was given."""
    L = capi.lib()
    i32, i64, f64 = [C.c_int32(7) for _ in range(6)], [C.c_int64(7) for _ in range(2)], C.c_double(7)
    buf = np.full((5, 4), 7, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for pre in ("slideo_matcher_", "slideo_group_"):
        assert getattr(L, pre + "placement_begin")(None, 32, 0, C.c_double(3.0)) == 1
        assert getattr(L, pre + "placement_end")(None) == 1
        assert getattr(L, pre + "placement_info")(None, C.byref(i32[0]), C.byref(i32[1]), C.byref(f64), *[C.byref(v) for v in i32[2:6]], C.byref(i64[0])) == 1
        assert getattr(L, pre + "placement_sums")(None, *[p(buf[i]) for i in range(5)], C.c_int64(4), C.byref(i32[0]), C.byref(i32[1]), C.byref(i64[0]),
                                                  C.byref(i64[1])) == 1
    assert all(v.value == 7 for v in i32 + i64) and f64.value == 7 and (buf == 7).all()


# ---- slideo_placement_quad -----------------------------------------------------------------------------------------------------------
AW, AH = 960, 540


def _true_h(quad):
    """unit slide -> pixels for a quad given as four corners."""
    return P.quad_homography(quad, 2, 2)                       # (a 2 x 2 page: its corner pixel centres are the unit square's corners)


QUADS = [((40.0, 24.0), (920.0, 50.0), (908.0, 492.0), (52.0, 520.0)), ((200.0, 100.0), (700.0, 100.0), (700.0, 400.0), (200.0, 400.0)),
         ((310.5, 20.25), (900.0, 150.5), (820.75, 500.0), (120.0, 380.5))]


def _compare(capi, sm, cell, min_count, trim, rounds, guard=True):
    want = P.quad(sm, cell, AW, AH, min_count, trim, rounds, guard=guard)
    if want is None:
        with pytest.raises(capi.SlideoError) as e:
            capi.placement_quad(sm, cell, AW, AH, min_count, trim, rounds)
        assert e.value.code == 1
        return None
    q, H, used, rms = capi.placement_quad(sm, cell, AW, AH, min_count, trim, rounds)
    err = float(np.abs(np.array(q) - want[0]).max())
    assert err <= 1e-3, err
    assert used == len(want[2]) and abs(rms - want[3]) <= 1e-3
    assert np.abs(H / H[2, 2] - want[1]).max() <= 1e-6 * max(1.0, np.abs(want[1]).max())
    return np.array(q), used, want


@pytest.mark.parametrize("cell", [16, 32, 64])
def test_quad_recovers_exact_homographies(capi, cell):
    rng = np.random.default_rng(31)
    for quad in QUADS:
        sm = P.sums_of_homography(_true_h(quad), AW, AH, cell, (3, 40), rng)
        q, used, want = _compare(capi, sm, cell, 1, 2.0, 4)
        # the cells hold exact correspondences up to the sums' own rounding (2^-20 of a slide about 1000 px long, 1/16 px)
        assert np.abs(q - np.array(quad)).max() < 0.05, (quad, q)
        assert used == int((sm[0] > 0).sum()) and used >= 12
        # min_count leaves out the cells below it
        q2, used2, _ = _compare(capi, sm, cell, 20, 2.0, 0)
        assert used2 == int((sm[0] >= 20).sum()) < used


def test_quad_trims_outlier_cells(capi):
    rng = np.random.default_rng(32)
    quad = QUADS[0]
    sm = P.sums_of_homography(_true_h(quad), AW, AH, 32, 10, rng)
    inl = np.argwhere(sm[0] > 0)
    bad = inl[rng.choice(len(inl), 5, replace=False)]
    for k, (cy, cx) in enumerate(bad):                          # a cell's slide position moved by 1 .. 2.6 % of the slide (9 .. 23 px)
        sm[3, cy, cx] += np.uint64(10 * int((0.010 + 0.004 * k) * 1048576))
    # (5 of 405 unweighted points 9 .. 23 px off move a least-squares fit by well under the 2 px trim: every true cell survives round 1)
    untrimmed = capi.placement_quad(sm, 32, AW, AH, 1, 2.0, 0)
    assert np.abs(np.array(untrimmed[0]) - np.array(quad)).max() > 0.05 and untrimmed[2] == len(inl)
    q, used, want = _compare(capi, sm, 32, 1, 2.0, 8)
    assert used == len(inl) - 5 and np.abs(q - np.array(quad)).max() < 0.05
    kept = set(want[2])
    assert all((int(cy), int(cx)) not in kept for cy, cx in bad)
    # dropped cells do not come back: gross outliers bend the first fit and take true cells with them; the kept set is the restatement's
    for k, (cy, cx) in enumerate(bad):
        sm[3, cy, cx] += np.uint64(10 * int(0.08 * 1048576))
    q, used, want = _compare(capi, sm, 32, 1, 2.0, 8)
    assert 4 <= used < len(inl) - 5


def test_quad_refuses_what_determines_no_homography(capi):
    L = capi.lib()
    rng = np.random.default_rng(33)
    H = _true_h(QUADS[0])
    full = P.sums_of_homography(H, AW, AH, 32, 5, rng)
    cells = np.argwhere(full[0] > 0)

    def only(sel):
        sm = np.zeros_like(full)
        for cy, cx in sel:
            sm[:, cy, cx] = full[:, cy, cx]
        return sm
    three = only(cells[[0, 40, 200]])
    row = only([c for c in cells if c[0] == cells[len(cells) // 2][0]])          # one row of cells on one slide row: collinear in both
    row[4] = row[0] * np.uint64(1 << 19)
    assert int((row[0] > 0).sum()) >= 8
    line_uv = np.zeros_like(full)                                               # distinct frame cells, collinear slide points
    for k, (cy, cx) in enumerate(cells[::7][:12]):
        t = 0.1 + 0.06 * k
        line_uv[:, cy, cx] = [4, 4 * int((cx * 32 + 16) * 16), 4 * int((cy * 32 + 16) * 16), 4 * int(t * 1048576), 4 * int(t * 1048576)]
    for sm in (three, row, line_uv, np.zeros_like(full)):
        assert _compare(capi, sm, 32, 1, 2.0, 4) is None
    four = only(cells[[0, 25, 180, 230]])
    assert _compare(capi, four, 32, 1, 2.0, 0) is not None                      # four cells in general position are enough
    assert _compare(capi, full, 32, 6, 2.0, 4) is None                          # min_count leaves nothing
    # trimming down to fewer than 4: outliers everywhere
    wild = full.copy()
    wild[3] = (wild[3].astype(np.float64) * rng.uniform(0.2, 1.0, wild[3].shape)).astype(np.uint64)
    assert _compare(capi, wild, 32, 1, 0.01, 8, guard=False) is None
    # bad arguments: nothing is written
    out, Ho = np.full(8, 7.0), np.full(9, 7.0)
    used, rms = C.c_int32(7), C.c_double(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    gh, gw = full.shape[1:]

    def call(sm=full, gw_=gw, gh_=gh, cell=32, aw=AW, ah=AH, mc=1, trim=2.0, rounds=4, q=out, drop=None):
        arr = [p(sm[i]) for i in range(5)]
        if drop is not None:
            arr[drop] = None
        return L.slideo_placement_quad(*arr, gw_, gh_, cell, aw, ah, C.c_int64(mc), C.c_double(trim), rounds, p(q), p(Ho), C.byref(used), C.byref(rms))
    over = full.copy(); over[1, cells[0][0], cells[0][1]] = full[0, cells[0][0], cells[0][1]] * np.uint64(65536) + np.uint64(1)
    for kw in (dict(drop=0), dict(drop=4), dict(q=None), dict(cell=24), dict(gw_=gw + 1), dict(gh_=gh - 1), dict(aw=0), dict(ah=5000), dict(mc=0),
               dict(trim=0.0), dict(trim=-1.0), dict(trim=float("nan")), dict(trim=float("inf")), dict(rounds=-1), dict(rounds=9), dict(sm=over),
               dict(sm=three), dict(sm=row)):
        assert call(**kw) == 1, kw
    assert (out == 7).all() and (Ho == 7).all() and used.value == 7 and rms.value == 7
    assert call() == 0 and used.value == len(cells)
    with pytest.raises(ValueError):
        capi.placement_quad(full[:4], 32, AW, AH, 1, 2.0, 4)


# ---- tools/placement_hostcheck.cpp -----------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "placement_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("placement"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("placement_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


_traces = {}


def _oracle_unit(oracle, name, fa, pset):
    """A constructed case through the CPU restatement of the pipeline: (cfg, frames of placement_ref.sums, train_page, page_xy, page
    sizes).  A page set is a deck of the selected pages alone; its page indices and train rows are mapped back to the whole deck's."""
    if name in _traces:
        return _traces[name]
    case = VC.build(*fa)
    cfg = small_cfg(oracle, **case.cfg)
    train, tp, pxy = case.deck()
    sel = list(range(len(case.pages))) if pset is None else sorted(pset)
    db = oracle.PageDB(cfg)
    sizes = {i: T.page_size(case, i) for i in range(len(case.pages))}
    for i in sel:
        pg = case.pages[i]
        w, h = sizes[i]
        db.add_page_features(w, h, VC.keypoints(pg.xy), pg.desc, oracle.small_image(T.page_pixels(case, i), cfg.small_area))
    assert db.finalize() == 0
    rows = None if pset is None else np.nonzero(np.isin(tp, sel))[0]
    frames = []
    for fi, f in enumerate(case.frames):
        v, cands = db.match_features_trace(case.frame_pixels(fi), VC.keypoints(f.xy), f.desc)
        cands = [{"page_idx": sel[int(c["page_idx"])], "transform": c["transform"], "n_votes": int(c["n_votes"]), "inliers": int(c["inliers"])}
                 for c in cands]
        rec = P.frame_record(cfg, f.xy, f.desc, cands, train, rows)
        rec["order"] = [(c["page_idx"], c["n_votes"]) for c in cands]
        frames.append(rec)
    _traces[name] = (cfg, frames, tp, pxy, sizes)
    return _traces[name]


def _write_unit(path, cfg, frames, tp, pxy, sizes, min_inliers, cell, reach, flags=0, rerun_mask=12, shuffle=None):
    """The unit as the device holds it: the votes of a frame at qofs[f] * k, a candidate's run at its ofs, in candidate order.
    shuffle: a generator that permutes the votes inside every run (the stored order must not matter)."""
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
            if shuffle is not None:
                run = [run[i] for i in shuffle.permutation(len(run))]
            base = int(qofs[fi]) * k + at
            votes[base:base + len(run)] = np.array(run, np.uint32).reshape(-1, 2)
            M = np.asarray(M, np.float64)
            tail += struct.pack("<5i", page, len(run), at, inliers, int(np.any(M != 0))) + M.tobytes()
            at += len(run)
    kp = np.concatenate([VC.keypoints(f["xy"]) for f in frames]) if qtot else np.zeros(0, VC.KEYPOINT_DTYPE)
    npages = int(tp.max()) + 1
    with open(path, "wb") as o:
        o.write(struct.pack("<16i", cfg.verify_model, k, VC.FRAME_W, VC.FRAME_H, min_inliers, cell, 0, len(frames), len(tp), qtot, flags, rerun_mask, npages,
                            0, 0, 0))
        o.write(struct.pack("<d", reach))
        o.write(qofs.tobytes()); o.write(kp.tobytes())
        o.write(np.ascontiguousarray(pxy, np.float32).tobytes()); o.write(votes.tobytes()); o.write(tail)
        for p in range(npages):
            o.write(struct.pack("<2i", *sizes.get(p, (1, 1))))


def _host_sums(exe, tmp, unit_args, cell, **kw):
    unit, out = str(tmp / "unit.bin"), str(tmp / "out.bin")
    _write_unit(unit, *unit_args, **kw)
    stats = subprocess.check_output([exe, unit, out]).decode().split()
    got = np.fromfile(out, np.uint64)
    gw, gh = E.grid(VC.FRAME_W, VC.FRAME_H, cell)
    assert got.size == 5 * gw * gh + 1
    return got[:-1].reshape(5, gh, gw), int(got[-1]), dict(zip(stats[::2], map(int, stats[1::2])))


def _check_cases(oracle, exe, tmp):
    windows = 0
    for name, fa, pset, min_inliers in P.constructed_cases():
        cfg, frames, tp, pxy, sizes = _oracle_unit(oracle, name, fa, pset)
        for cell, reach in ((16, P.REACHES[0]), (32, P.REACHES[0]), (64, P.REACHES[0]), (32, P.REACHES[1])):
            stats = {}
            want = P.sums(frames, cell=cell, aw=VC.FRAME_W, ah=VC.FRAME_H, min_inliers=min_inliers, reach=reach, model=cfg.verify_model, train_page=tp,
                          page_xy=pxy, page_sizes=sizes, stats=stats)                  # (asserts the guards on every tested d2)
            got, counted, hs = _host_sums(exe, tmp, (cfg, frames, tp, pxy, sizes, min_inliers, cell, reach), cell)
            assert np.array_equal(got, want[0]) and counted == want[2], (name, cell, reach)
            shuffled, counted2, _ = _host_sums(exe, tmp, (cfg, frames, tp, pxy, sizes, min_inliers, cell, reach), cell, shuffle=np.random.default_rng(5))
            assert np.array_equal(shuffled, got) and counted2 == counted, (name, "the votes' order entered")
            P.check_statements(name, reach, stats, want[0], want[2])
            windows = max(windows, hs["windows"])
    assert windows >= 2                                                              # (R2, H1: frames of more keypoints than a window)
    # a unit whose run raised a re-run bit counts nothing
    name, fa, pset, mi = P.constructed_cases()[0]
    cfg, frames, tp, pxy, sizes = _oracle_unit(oracle, name, fa, pset)
    for flags, mask, counts in ((4, 12, False), (8, 12, False), (8, 4, True), (2, 12, True)):
        got, counted, _ = _host_sums(exe, tmp, (cfg, frames, tp, pxy, sizes, mi, 32, 8.0), 32, flags=flags, rerun_mask=mask)
        assert bool(got.sum()) == counts and bool(counted) == counts, (flags, mask)


def test_host_build_of_the_kernel_body_equals_the_restatement(oracle, hostcheck, tmp_path):
    _check_cases(oracle, hostcheck, tmp_path)


def test_sanitized_host_build_over_the_constructed_cases(oracle, hostcheck_san, tmp_path):
    """Address and undefined-behaviour checks with every array in an allocation of exactly its size.  A stand-alone program: nothing
    is loaded into Python."""
    _check_cases(oracle, hostcheck_san, tmp_path)


def test_wild_features_reach_no_counter(oracle, hostcheck_san, tmp_path):
    """A caller's own features may hold any float: keypoints and transforms that give negative, huge, infinite or NaN positions count
    nowhere and store nothing outside the grid (the sanitized build)."""
    name, fa, pset, mi = P.constructed_cases()[0]
    cfg, frames, tp, pxy, sizes = _oracle_unit(oracle, name, fa, pset)
    slot = T.contributor(frames[0]["cands"], 0)
    for k, wild in enumerate(([1e300, 0, 0, 0, 1e300, 0], [np.nan] * 6, [np.inf, 0, 5, 0, -np.inf, 5], [1, 0, -1e9, 0, 1, 2.0 ** 40])):
        f = dict(frames[0])
        f["cands"] = list(f["cands"])
        M = np.array(f["cands"][slot][2], np.float64, copy=True)
        M[:6] = wild
        f["cands"][slot] = (f["cands"][slot][0], f["cands"][slot][1], M)
        want = P.sums([f], cell=16, aw=VC.FRAME_W, ah=VC.FRAME_H, min_inliers=mi, reach=1e6, model=cfg.verify_model, train_page=tp, page_xy=pxy,
                      page_sizes=sizes, guard=False)
        got, counted, _ = _host_sums(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, sizes, mi, 16, 1e6), 16)
        assert np.array_equal(got, want[0]) and counted == want[2], k
    f = dict(frames[0]); f["xy"] = np.array(f["xy"], np.float32, copy=True)
    f["xy"][:7] = [[-0.5, 10], [10, -3e9], [1e30, 10], [10, 360], [np.nan, 10], [np.inf, -np.inf], [639.99, 359.99]]
    want = P.sums([f], cell=16, aw=VC.FRAME_W, ah=VC.FRAME_H, min_inliers=mi, reach=1e6, model=cfg.verify_model, train_page=tp, page_xy=pxy,
                  page_sizes=sizes, guard=False)
    got, counted, _ = _host_sums(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, sizes, mi, 16, 1e6), 16)
    assert np.array_equal(got, want[0]) and counted == want[2] == 1 and got[0].sum() > 0


# ---- the use -------------------------------------------------------------------------------------------------------------------------

def test_the_use_on_the_cpu(capi, oracle, synth):
    """The keystone scene (tests/placement_ref.py keystone_scene: the canvas texture with the four glyph pages shown over one fixed
    keystoned quad, 8 frames, ORB-3000, min_rating 12) through the CPU restatement of the pipeline, evidence_ref.votes_of and
    placement_ref at cell 32, min_inliers 12, reach 24, min_count 2, trim 3 px, 4 rounds:
      - at least half of the frames have a contributor;
      - the kept cells span at least three quarters of the slide along u and along v;
      - the learnt quad's largest corner error against the scene's quad is within USE["bound_px"], which is twice the value measured
        here rounded up to a whole pixel.
    The library's slideo_placement_quad gives the restatement's quad on these sums.
    Measured: 8 of 8 frames contribute; the largest corner error is 1.24 px (docs/EXTENSIONS.md "Match placement map")."""
    pages, frames, truth = P.keystone_scene(synth)
    U = P.USE
    cfg = small_cfg(oracle, nfeatures=U["nfeatures"], min_rating=U["min_rating"])
    db = oracle.PageDB(cfg)
    db.add_pages(pages, threads=4)
    assert db.finalize() == 0
    train = db.train()
    tp, pxy = E.deck_of(db, len(pages))
    sizes = {p: (pages[p].shape[1], pages[p].shape[0]) for p in range(len(pages))}
    recs = []
    for f in frames:
        _, cands = db.match_frame_trace(f)
        kp, desc = oracle.orb(f, cfg)
        recs.append(P.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, cands, train))
    sm, through, counted = P.sums(recs, cell=U["cell"], aw=E.CANVAS_W, ah=E.CANVAS_H, min_inliers=U["min_inliers"], reach=U["reach"], model=0,
                                  train_page=tp, page_xy=pxy, page_sizes=sizes, guard=False)
    want = P.quad(sm, U["cell"], E.CANVAS_W, E.CANVAS_H, U["min_count"], U["trim"], U["rounds"], guard=False)
    assert want is not None
    q, H, used, rms = capi.placement_quad(sm, U["cell"], E.CANVAS_W, E.CANVAS_H, U["min_count"], U["trim"], U["rounds"])
    assert np.abs(np.array(q) - want[0]).max() <= 1e-3 and used == len(want[2])
    err = P.corner_error(q)
    su, sv = P.span_of(sm, want[2], U["cell"], U["min_count"])
    print("the use on the CPU: %d of %d frames contribute, %d keypoints in %d kept cells, rms %.2f px, span %.2f x %.2f, largest corner error %.2f px"
          % (counted, through, int(sm[0].sum()), used, rms, su, sv, err))
    assert 2 * counted >= through
    assert su >= 0.75 and sv >= 0.75
    assert err <= U["bound_px"] and U["bound_px"] == math.ceil(2 * 1.24)
