"""The gate settle (include/slideo_amd.h "Gate settle") on a CPU-only box: the header declares the section and the calls, the library
exports them at ABI 7, null handles are refused before the device, the mirrors name the option, the numpy restatement
(tests/gate_settle_ref.py) does on a stream of holds, hard cuts, fades and a noisy hold what the rule was made for, and
tools/gate_settle_hostcheck.cpp — a program with its own main, built with the host compiler, plain and under
-fsanitize=address,undefined; nothing sanitized is loaded into Python — holds the proposal's ranges, the rule against both gate
references, the group rule and a plain C++ restatement of the walk kernel's 64-lane window to values this file computes with the
numpy restatement."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gate_anchor_ref as aref
import gate_mask_ref as gref
import gate_settle_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["slideo_matcher_set_gate_settle", "slideo_matcher_gate_settle", "slideo_group_set_gate_settle", "slideo_small_carried_ssd",
         "slideo_gate_settle_walk"]
CS = 0.98                                                        # cfg.changed_similarity's default
SETTLE = 0.99
NEVER = 2 ** 30                                                  # a deferral cap no stream here reaches


def test_header_declares_the_gate_settle():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "---- Gate settle (" in src
    sec = src[src.index("---- Gate settle ("):]
    sec = sec[:sec.index("/* ---- Direct page look-up")]
    for words in ("settle_similarity == 0 is off", "away = ssd_a >= T_c, still = ssd_p < T_s", "away && (still || d >= max_defer)",
                  "d = min(d + 1, max_defer)", "changed == 0 && similarity < cfg.changed_similarity", "With max_defer == 0 the rule is ANCHOR, bit for bit",
                  "at most max_defer", "SECOND frame of the new hold", "holds are one frame long", "SLIDEO_ERR_UNSUPPORTED"):
        assert words in sec, words
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name
    assert "#define SLIDEO_ABI_VERSION 7" in src
    assert not re.search(r"#define SLIDEO_GATE_\w+\s+2u", src), "the gate reference keeps its two values"


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    for cls in (capi.Matcher, capi.Group):
        assert callable(cls.set_gate_settle) and callable(cls.gate_settle)
    assert callable(capi.Matcher.small_carried_ssd) and callable(capi.Matcher.gate_settle_walk)


def test_null_handles_and_the_binding_refuse_before_the_device(capi):
    L = capi.lib()
    s, d = C.c_float(7.0), C.c_int32(7)
    buf = (C.c_uint8 * 64)()
    assert L.slideo_matcher_set_gate_settle(None, 0.99, 4) == 1
    assert L.slideo_matcher_set_gate_settle(None, 5.0, -1) == 1
    assert L.slideo_matcher_gate_settle(None, C.byref(s), C.byref(d)) == 1 and (s.value, d.value) == (7.0, 7)
    assert L.slideo_group_set_gate_settle(None, 0.99, 4) == 1
    assert L.slideo_small_carried_ssd(None, buf, buf, buf, 1, 2, 2, 0, buf) == 1
    assert L.slideo_gate_settle_walk(None, buf, buf, buf, 1, 0, 0, 0, 0, 0, buf, buf, buf, buf) == 1
    obj = capi.Matcher.__new__(capi.Matcher)                     # no handle, no device: the binding's own range check comes first
    obj._h = C.c_void_p()
    for bad in (-1, 2 ** 31):
        with pytest.raises(capi.SlideoError) as e:
            obj.set_gate_settle(0.99, bad)
        assert e.value.code == 1
    obj._h = None


def test_the_deferred_mask_helper(capi):
    changed = np.array([1, 0, 0, 0, 1], np.uint8)
    sims = np.array([0.0, 0.999, 0.97, 0.98, 0.5], np.float32)
    assert capi.gate_deferred(changed, sims, CS).tolist() == [False, False, True, False, False]


def test_mirrors_name_the_option():
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS[:3]:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    lib = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    assert "pub gate_settle: (f32, i32)" in lib and "gate_settle: (0.0, 0)" in lib and "pub fn gate_settle(mut self" in lib
    assert "ffi::slideo_group_set_gate_settle(h, self.gate_settle.0, self.gate_settle.1)" in lib
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_gate_settle(float settle_similarity, int32_t max_defer)" in hpp
    assert "slideo_group_set_gate_settle(h->g, settle_similarity_, settle_max_defer_)" in hpp
    from slideo_amd import matching
    assert "gate_settle" in inspect.signature(matching.HipImageVideoMatcher.__init__).parameters
    # the gated flush emits the frames with a verdict only: a deferred frame (changed == 0) is skipped like an unchanged one
    src = inspect.getsource(matching)
    assert "set_gate_settle(*self._gate_settle)" in src


def test_the_setting_did_not_grow():
    fs = open(os.path.join(ROOT, "slideo_amd", "csrc", "frame_settings.h")).read()
    enum = re.search(r"enum Setting \{(.*?)\}", fs, re.S).group(1)
    names = [n.strip() for n in enum.split(",") if n.strip()]
    assert names[-2:] == ["SET_GATE_REFERENCE", "N_SETTINGS"] and len(names) == 9


# ---- the restatement on a stream of holds, hard cuts, two fades and a noisy hold -----------------------------------------------------
def _fade(a, b, k):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return [a, a, a] + [np.rint(a64 + (b64 - a64) * j / k).astype(np.uint8) for j in range(1, k)] + [b, b, b]


@pytest.fixture(scope="module")
def stream(oracle, cfg0_data):
    """-> (small images [n], holds: (first, last) frame of each, fades: (first, last) inner frame of each)."""
    _, f, _, _ = cfg0_data
    rng = np.random.default_rng(19)
    seq, holds, fades = [], [], []

    def hold(frames):
        holds.append((len(seq), len(seq) + len(frames) - 1))
        seq.extend(frames)

    hold([f[0]] * 4)
    fd = _fade(f[1], f[2], 24)                                   # a hard cut into the first hold of the fade
    hold([f[1]] + fd[:3])
    fades.append((len(seq), len(seq) + 22))
    seq.extend(fd[3:26])
    hold(fd[26:])
    hold([f[3]] * 4)                                             # hard cuts on both sides
    fd = _fade(f[4], f[5], 24)
    hold(fd[:3])
    fades.append((len(seq), len(seq) + 22))
    seq.extend(fd[3:26])
    hold(fd[26:])
    hold([np.clip(f[6].astype(np.int16) + rng.integers(-3, 4, f[6].shape), 0, 255).astype(np.uint8) for _ in range(6)])
    smalls = gref.small_images(oracle, seq)
    return smalls, holds, fades


def test_the_stream_is_what_the_rule_was_made_for(stream):
    smalls, holds, fades = stream
    n = smalls.shape[1] * smalls.shape[2]
    valid = np.ones(smalls.shape[1:3], bool)
    cons = np.array([gref.similarity(gref.masked_ssd(smalls[i - 1], smalls[i], valid), n) for i in range(1, len(smalls))])
    inside = np.zeros(len(smalls), bool)                         # frame i differs from frame i - 1 by one step of a fade
    for lo, hi in fades:
        inside[lo:hi + 2] = True
    print("consecutive similarity: %.4f .. %.4f inside the fades, >= %.4f in the holds" % (cons[inside[1:]].min(), cons[inside[1:]].max(),
                                                                                          min(cons[lo:hi].min() for lo, hi in holds)))
    assert cons[inside[1:]].max() < np.float32(SETTLE), "every step of a fade is not still"
    for lo, hi in holds:
        assert cons[lo:hi].min() >= np.float32(SETTLE), "inside a hold, the noisy one too, the picture stands still"


def test_max_defer_0_is_the_anchor_rule(stream):
    smalls, _, _ = stream
    ch, sim, kind, _, state = sref.flags(smalls, None, CS, SETTLE, 0)
    ach, asim, _, alast = aref.flags(smalls, None, CS)
    assert np.array_equal(ch, ach) and sim.tobytes() == asim.tobytes() and np.array_equal(state[0], alast)
    assert not (kind == sref.DEFERRED).any()
    assert np.array_equal(state[1], smalls[-1]) and state[2] == 0


def test_without_a_cap_every_hold_is_matched_once_and_no_fade_frame(stream):
    smalls, holds, fades = stream
    ch, sim, kind, _, state = sref.flags(smalls, None, CS, SETTLE, NEVER)
    ach = aref.flags(smalls, None, CS)[0]
    print("ANCHOR matches %d of %d frames, the settle %d: %s" % (ach.sum(), len(smalls), ch.sum(), np.nonzero(ch)[0].tolist()))
    for lo, hi in holds:
        assert ch[lo:hi + 1].sum() == 1, "hold %d .. %d" % (lo, hi)
    for lo, hi in fades:
        assert not ch[lo:hi + 1].any() and (kind[lo:hi + 1] == sref.DEFERRED).any(), "fade %d .. %d" % (lo, hi)
    assert int(ch.sum()) == len(holds) < int(ach.sum())
    assert not (kind == sref.MATCHED_CAP).any()
    # a hard cut is matched on the second frame of the new hold; the state "none" on the first
    assert np.nonzero(ch)[0].tolist() == [holds[0][0]] + [lo + 1 for lo, _ in holds[1:]]
    # a deferred frame is recognisable from the two outputs alone
    assert np.array_equal(kind == sref.DEFERRED, ~ch & (sim < np.float32(CS)))
    assert np.array_equal(state[0], smalls[holds[-1][0] + 1])


def test_a_cap_of_4_matches_inside_the_fades(stream):
    smalls, _, fades = stream
    ch, sim, kind, d, _ = sref.flags(smalls, None, CS, SETTLE, 4)
    cap = np.nonzero(kind == sref.MATCHED_CAP)[0]
    assert len(cap) >= 1 and (d[cap] == 4).all(), "at least one frame is matched by the cap: away, not still, d == 4"
    assert all(any(lo <= i <= hi + 1 for lo, hi in fades) for i in cap)
    assert (d <= 4).all()
    # a change of any length gets a verdict at most max_defer frames after it began: no run of deferred frames is longer than 4
    run = 0
    for k in kind:
        run = run + 1 if k == sref.DEFERRED else 0
        assert run <= 4


@pytest.mark.parametrize("max_defer", [NEVER, 4])
def test_cutting_the_stream_changes_nothing(stream, max_defer):
    smalls, _, _ = stream
    ch, sim, kind, d, state = sref.flags(smalls, None, CS, SETTLE, max_defer)
    for cut in (1, 7, 20):
        c0, s0, k0, d0, st0 = sref.flags(smalls[:cut], None, CS, SETTLE, max_defer)
        c1, s1, k1, d1, st1 = sref.flags(smalls[cut:], None, CS, SETTLE, max_defer, st0)
        assert np.array_equal(np.concatenate([c0, c1]), ch) and np.concatenate([s0, s1]).tobytes() == sim.tobytes()
        assert np.array_equal(np.concatenate([k0, k1]), kind) and np.array_equal(np.concatenate([d0, d1]), d)
        assert np.array_equal(st1[0], state[0]) and np.array_equal(st1[1], state[1]) and st1[2] == state[2]


def test_the_integer_walk_is_the_rule(stream):
    """gate_settle_ref.walk over the table of all pairs = gate_settle_ref.flags over the images, whole stream and from a carried state."""
    smalls, _, _ = stream
    n = smalls.shape[1] * smalls.shape[2]
    valid = np.ones(smalls.shape[1:3], bool)
    t_c, t_s = gref.threshold(CS, n), gref.threshold(SETTLE, n)
    assert 0 < t_s < t_c
    table = aref.all_pairs_ssd(smalls)
    for max_defer in (NEVER, 4):
        ch, _, kind, d, state = sref.flags(smalls, None, CS, SETTLE, max_defer)
        fl, ssd, wkind, last, d_out = sref.walk(table, np.zeros(len(smalls) + 1, np.int64), t_c, t_s, max_defer, 0, True)
        assert np.array_equal(fl.astype(bool), ch) and np.array_equal(wkind, kind) and last == np.nonzero(ch)[0].max() and d_out == state[2]
        cut = 20
        _, _, _, _, st0 = sref.flags(smalls[:cut], None, CS, SETTLE, max_defer)
        assert max_defer != NEVER or st0[2] > 0, "without a cap the cut falls inside a run of deferred frames"
        carried = np.array([gref.masked_ssd(st0[0], s, valid) for s in smalls[cut:]] + [gref.masked_ssd(st0[1], smalls[cut], valid)], np.int64)
        fl, ssd, wkind, last, d_out = sref.walk(table[cut:, cut:], carried, t_c, t_s, max_defer, st0[2], False)
        assert np.array_equal(fl.astype(bool), ch[cut:]) and np.array_equal(wkind, kind[cut:]) and d_out == state[2]


# ---- the host check ---------------------------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(20261019)
    out = []
    for n in (1, 2, 63, 64, 65, 130):
        for none in (0, 1):
            for max_defer in (0, 1, 3, 70, NEVER):
                for p_away, p_still in ((0.0, 0.5), (1.0, 0.0), (1.0, 1.0), (0.9, 0.1), (0.5, 0.5), (0.97, 0.02)):
                    table = rng.integers(0, 1 << 40, (n, n), dtype=np.int64)
                    carried = rng.integers(0, 1 << 40, n + 1, dtype=np.int64)
                    thr_c = {0.0: (1 << 63) - 1, 1.0: 0}.get(p_away, int((1 << 40) * (1.0 - p_away)))
                    thr_s = {0.0: 0, 1.0: (1 << 63) - 1}.get(p_still, int((1 << 40) * p_still))
                    d_in = 0 if none else int(rng.integers(0, min(max_defer, 80) + 1))
                    fl, ssd, kind, last, d_out = sref.walk(table, carried, thr_c, thr_s, max_defer, d_in, bool(none))
                    out.append((n, thr_c, thr_s, max_defer, d_in, none, carried, table, fl, ssd, kind, last, d_out))
    return out


def test_host_check_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    cases = _cases()
    kinds = np.concatenate([c[10] for c in cases])
    assert all((kinds == k).any() for k in (sref.UNCHANGED, sref.DEFERRED, sref.MATCHED_STILL, sref.MATCHED_CAP)), "every branch occurs"
    assert any((c[10] == sref.DEFERRED).all() and c[0] > 64 for c in cases), "a run of deferred frames crosses the 64-lane window"
    assert any(c[3] == 70 and (c[10] == sref.MATCHED_CAP).any() and c[0] > 70 for c in cases), "the cap is reached behind a window's end"
    assert any(c[4] > 0 for c in cases)
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for n, thr_c, thr_s, max_defer, d_in, none, carried, table, fl, ssd, kind, last, d_out in cases:
            f.write("%d %d %d %d %d %d\n" % (n, thr_c, thr_s, max_defer, d_in, none))
            for arr in (carried, table.reshape(-1), fl, ssd):
                f.write(" ".join(str(int(v)) for v in arr) + "\n")
            f.write("%d %d\n" % (last, d_out))
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
            os.path.join(ROOT, "tools", "gate_settle_hostcheck.cpp")]
    for tag, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("hostcheck_" + tag))
        subprocess.check_call(base + extra + ["-o", exe])
        out = subprocess.check_output([exe, path]).decode()
        assert "%d walks: as stated" % len(cases) in out, out


def test_the_frame_settings_host_check_still_walks_144_pairs(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "fs_hostcheck")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_settings_hostcheck.cpp"), "-o", exe])
    assert "144 ordered pairs" in subprocess.check_output([exe]).decode()
