"""The gate reference (include/slideo_amd.h "Gate reference") on a CPU-only box: the header declares the calls and the library exports
them at ABI 7, the mirrors name the option, the numpy restatement (tests/gate_anchor_ref.py) does on hand-checked streams what the
rule was made for, and tools/gate_anchor_hostcheck.cpp — a program with its own main, built with the host compiler, plain and under
-fsanitize=address,undefined; nothing sanitized is loaded into Python — holds the proposal's refusals, the SETTING_ENDS row, the
group rule and a plain C++ walk over random SSD tables to values this file computes with the restatement."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gate_anchor_ref as aref
import gate_mask_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["slideo_matcher_set_gate_reference", "slideo_matcher_gate_reference", "slideo_group_set_gate_reference", "slideo_small_gram_ssd"]
CS = 0.98                                                        # cfg.changed_similarity's default


def test_header_declares_the_gate_reference():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Gate reference" in src and "MarkSimilarIter, whatever the gate reference is" in src
    assert re.search(r"#define SLIDEO_GATE_PREVIOUS\s+0u", src) and re.search(r"#define SLIDEO_GATE_ANCHOR\s+1u", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    assert (capi.GATE_PREVIOUS, capi.GATE_ANCHOR) == (0, 1)
    for cls in (capi.Matcher, capi.Group):
        assert callable(cls.set_gate_reference) and callable(cls.gate_reference)
    assert callable(capi.Matcher.small_gram_ssd)


def test_null_handles_and_the_binding_refuse_before_the_device(capi):
    L = capi.lib()
    ref = C.c_uint32(7)
    buf = (C.c_uint8 * 64)()
    assert L.slideo_matcher_set_gate_reference(None, 1) == 1
    assert L.slideo_matcher_set_gate_reference(None, 99) == 1
    assert L.slideo_matcher_gate_reference(None, C.byref(ref)) == 1 and ref.value == 7
    assert L.slideo_group_set_gate_reference(None, 1) == 1
    assert L.slideo_small_gram_ssd(None, buf, 1, 2, 2, 0, buf) == 1
    obj = capi.Matcher.__new__(capi.Matcher)                     # no handle, no device: the binding's own check of a name comes first
    obj._h = C.c_void_p()
    with pytest.raises(capi.SlideoError) as e:
        obj.set_gate_reference("settle")
    assert e.value.code == 1
    obj._h = None


def test_mirrors_name_the_option():
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert "pub const SLIDEO_GATE_PREVIOUS: u32 = 0;" in ffi and "pub const SLIDEO_GATE_ANCHOR: u32 = 1;" in ffi
    lib = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    assert "pub gate_reference: u32" in lib and "gate_reference: ffi::SLIDEO_GATE_PREVIOUS" in lib
    assert "ffi::slideo_group_set_gate_reference(h, self.gate_reference)" in lib
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_gate_reference(uint32_t ref)" in hpp and "slideo_group_set_gate_reference(h->g, gate_ref_)" in hpp
    import inspect
    from slideo_amd import matching
    assert "gate_reference" in inspect.signature(matching.HipImageVideoMatcher.__init__).parameters


# ---- the restatement on hand-checked streams ----------------------------------------------------------------------------------------
def _fade(a, b, k):
    """Three copies of a, the k - 1 inner steps rint(a + (b - a) j / k), three copies of b."""
    a16, b16 = a.astype(np.float64), b.astype(np.float64)
    steps = [np.rint(a16 + (b16 - a16) * j / k).astype(np.uint8) for j in range(1, k)]
    return np.stack([a, a, a] + steps + [b, b, b])


@pytest.fixture(scope="module")
def fade_smalls(oracle, cfg0_data):
    _, frames, _, _ = cfg0_data
    return {k: gref.small_images(oracle, _fade(frames[1], frames[2], k)) for k in (8, 24)}


def test_the_fade_the_previous_rule_misses(fade_smalls):
    s = fade_smalls[24]
    assert s.shape[1:] == (259, 461, 3)
    n = 259 * 461
    assert gref.similarity(gref.masked_ssd(s[0], s[-1], np.ones((259, 461), bool)), n) < np.float32(0.75)     # two different slides
    prev, psim = gref.flags(s, None, CS)
    assert prev.tolist() == [True] + [False] * (len(s) - 1), "the PREVIOUS rule flags frame 0 and nothing else"
    assert psim[1:].min() >= np.float32(CS)
    ch, sim, ref, last = aref.flags(s, None, CS)
    print("anchor rule, k = 24: %d flagged: %s" % (ch.sum(), np.nonzero(ch)[0].tolist()))
    assert ch[0] and sim[0] == np.float32(0.0) and ref[0] == -1, "the state \"none\": frame 0 is flagged"
    fade = np.arange(3, 3 + 23)
    assert ch[fade].any(), "the anchor rule flags at least one frame of the fade"
    assert int(ch.sum()) == 13 and np.nonzero(ch)[0].tolist() == [0] + list(range(4, 27, 2)), "every second frame of the fade, up to the new slide"
    # the invariant: every unflagged frame is >= the threshold against its anchor, every flagged one <
    valid = np.ones((259, 461), bool)
    T = gref.threshold(CS, n)
    for i in range(1, len(s)):
        ssd = gref.masked_ssd(s[ref[i]], s[i], valid)
        assert sim[i] == gref.similarity(ssd, n)
        assert bool(ch[i]) == bool(sim[i] < np.float32(CS)) == (ssd >= T)
        assert ref[i] == np.nonzero(ch[:i])[0].max(), "the anchor is the last flagged frame before"
    # the stream ends on a verdict for the slide it ends on
    assert np.array_equal(last, s[np.nonzero(ch)[0].max()])
    assert gref.similarity(gref.masked_ssd(last, s[-1], valid), n) == np.float32(1.0)


def test_a_short_fade_is_flagged_by_both_rules(fade_smalls):
    s = fade_smalls[8]
    prev, _ = gref.flags(s, None, CS)
    ch, _, _, _ = aref.flags(s, None, CS)
    fade = np.arange(3, 3 + 8)                                   # the 7 inner steps and the first frame of the new slide
    assert prev[fade].all() and ch[fade].any()


def test_hard_cuts_give_the_same_flags(oracle, cfg0_data):
    _, frames, _, _ = cfg0_data
    smalls = gref.small_images(oracle, frames)
    order = [0, 0, 0, 1, 2, 2, 2, 2, 3, 4, 4, 5, 5, 5, 6, 7, 7, 0, 0, 3, 3]
    s = smalls[order]
    for start in (None, smalls[0], smalls[5]):
        prev, psim = gref.flags(s, None, CS, start)
        ch, sim, _, _ = aref.flags(s, None, CS, start)
        assert np.array_equal(prev, ch) and psim.tobytes() == sim.tobytes()
        cuts = np.array([True] + [order[i] != order[i - 1] for i in range(1, len(order))])
        if start is not None:
            cuts[0] = not np.array_equal(start, s[0])
        assert np.array_equal(ch, cuts)


def test_a_carried_anchor_and_a_mask(fade_smalls):
    """The walk continues from a carried anchor as from its own, and under a validity map the SSD runs over the valid pixels."""
    s = fade_smalls[24]
    valid = np.ones((259, 461), bool)
    valid[40:120, 300:440] = False
    ch, sim, ref, last = aref.flags(s, valid, CS)
    for cut in (1, 7, 20):
        c0, s0, _, a0 = aref.flags(s[:cut], valid, CS)
        c1, s1, r1, a1 = aref.flags(s[cut:], valid, CS, a0)
        assert np.array_equal(np.concatenate([c0, c1]), ch) and np.concatenate([s0, s1]).tobytes() == sim.tobytes()
        assert np.array_equal(a1, last)
        assert np.array_equal(np.where(r1 < 0, -1, r1 + cut)[r1 >= 0], ref[cut:][r1 >= 0])


# ---- the host check ---------------------------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(20261019)
    out = []
    for n in (1, 2, 63, 64, 65, 130, 300):
        for none in (0, 1):
            for density in (0.0, 0.02, 0.5, 1.0):
                table = rng.integers(0, 1 << 40, (n, n), dtype=np.int64)
                carried = rng.integers(0, 1 << 40, n, dtype=np.int64)
                thr = {0.0: (1 << 63) - 1, 1.0: 0}.get(density, int((1 << 40) * (1.0 - density)))
                fl, ssd, last = aref.walk(table, carried, thr, bool(none))
                out.append((n, thr, none, carried, table, fl, ssd, last))
    return out


def test_host_check_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    cases = _cases()
    assert any(c[5].all() for c in cases) and any(not c[5].any() for c in cases) and any(0 < c[5].sum() < len(c[5]) for c in cases)
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for n, thr, none, carried, table, fl, ssd, last in cases:
            f.write("%d %d %d\n" % (n, thr, none))
            for arr in (carried, table.reshape(-1), fl, ssd):
                f.write(" ".join(str(int(v)) for v in arr) + "\n")
            f.write("%d\n" % last)
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
            os.path.join(ROOT, "tools", "gate_anchor_hostcheck.cpp")]
    for tag, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("hostcheck_" + tag))
        subprocess.check_call(base + extra + ["-o", exe])
        out = subprocess.check_output([exe, path]).decode()
        assert "%d walks: as stated" % len(cases) in out, out
