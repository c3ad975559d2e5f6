"""The gate memory (include/slideo_amd.h "Gate memory") on a CPU-only box: the header declares the section, its sentences and the
calls, the library exports them at ABI 7, null handles are refused before the device, the mirrors name the option, the numpy
restatement (tests/gate_memory_ref.py) does on built streams what the rule was made for, the task's emission function is driven with
hand-made inputs, and tools/gate_memory_hostcheck.cpp — a program with its own main, built with the host compiler, plain and under
-fsanitize=address,undefined; nothing sanitized is loaded into Python — holds the proposal's ranges, the ANCHOR-only rule in both
call orders, the group rule, the record calls' refusal and a plain C++ restatement of the walk kernel's 64 lanes to values this file
computes with the numpy restatement."""
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
import gate_memory_cases as cases
import gate_memory_ref as mref
import gate_settle_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["slideo_matcher_set_gate_memory", "slideo_matcher_gate_memory", "slideo_group_set_gate_memory", "slideo_matcher_last_gate_refs",
         "slideo_group_last_gate_refs", "slideo_matcher_gate_memory_entries", "slideo_matcher_gate_memory_small", "slideo_gate_recall_walk"]
CS = 0.98                                                        # cfg.changed_similarity's default
SETTLE = 0.99
NEVER = 2 ** 30


def test_header_declares_the_gate_memory():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "---- Gate memory (" in src
    sec = src[src.index("---- Gate memory ("):]
    for words in ("0 is off", "1 <= M <= SLIDEO_GATE_MEMORY_MAX", "ties to the greatest", "FIFO: a recall does not refresh an entry",
                  "With M = 1, flags, similarities, verdicts, traces and the last small image equal those of the same stream without",
                  "Every frame with ref >= 0 is within cfg.changed_similarity of the frame with that ordinal",
                  "under whatever page set was selected then", "E = [(S, SLIDEO_GATE_REF_RESET)]", "ref = SLIDEO_GATE_REF_DEFERRED",
                  "a group of more than one member refuses M > 0 with SLIDEO_ERR_UNSUPPORTED", "_export / _import and the group forms return SLIDEO_ERR_UNSUPPORTED",
                  "M > 0 with a gate reference other than SLIDEO_GATE_ANCHOR is", "gate_recall_kernel", "gate_memory_state_kernel"):
        assert words in sec, words
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name
    assert "#define SLIDEO_ABI_VERSION 7" in src
    assert "#define SLIDEO_GATE_MEMORY_MAX 64" in src and "#define SLIDEO_GATE_REF_RESET (-1)" in src and "#define SLIDEO_GATE_REF_DEFERRED (-2)" in src
    assert not re.search(r"#define SLIDEO_GATE_\w+\s+2u", src), "the gate reference keeps its two values"


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    for cls in (capi.Matcher, capi.Group):
        assert callable(cls.set_gate_memory) and callable(cls.gate_memory) and callable(cls.last_gate_refs)
    for tap in ("gate_memory_entries", "gate_memory_small", "gate_recall_walk"):
        assert callable(getattr(capi.Matcher, tap))
    assert (capi.GATE_REF_RESET, capi.GATE_REF_DEFERRED, capi.GATE_MEMORY_MAX) == (-1, -2, 64)


def test_null_handles_and_the_binding_refuse_before_the_device(capi):
    L = capi.lib()
    c, n = C.c_int32(7), C.c_int64(7)
    buf = (C.c_uint8 * 1024)()
    assert L.slideo_matcher_set_gate_memory(None, 4) == 1
    assert L.slideo_matcher_set_gate_memory(None, 99) == 1
    assert L.slideo_matcher_gate_memory(None, C.byref(c)) == 1 and c.value == 7
    assert L.slideo_group_set_gate_memory(None, 4) == 1
    assert L.slideo_matcher_last_gate_refs(None, buf, 4, C.byref(n)) == 1 and n.value == 7
    assert L.slideo_group_last_gate_refs(None, buf, 4, C.byref(n)) == 1
    assert L.slideo_matcher_gate_memory_entries(None, C.byref(c), C.byref(c), buf) == 1
    assert L.slideo_matcher_gate_memory_small(None, 0, buf, 1024, C.byref(c), C.byref(c)) == 1
    assert L.slideo_gate_recall_walk(None, buf, buf, buf, buf, buf, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, buf, buf, buf, buf, buf, buf, buf, buf) == 1
    obj = capi.Matcher.__new__(capi.Matcher)                     # no handle, no device: the binding's own range check comes first
    obj._h = C.c_void_p()
    for bad in (-1, 65, 2 ** 31):
        with pytest.raises(capi.SlideoError) as e:
            obj.set_gate_memory(bad)
        assert e.value.code == 1
    obj._h = None


def test_mirrors_name_the_option():
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS[:5]:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    lib = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    assert "pub gate_memory: i32" in lib and "gate_memory: 0," in lib and "pub fn gate_memory(mut self" in lib
    assert "ffi::slideo_group_set_gate_memory(h, self.gate_memory)" in lib and "ffi::slideo_group_last_gate_refs(h" in lib
    assert "pub fn gate_memory_emission(" in lib
    assert lib.index("ffi::slideo_group_set_gate_settle(h") < lib.index("ffi::slideo_group_set_gate_memory(h"), "after the settle"
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_gate_memory(int32_t capacity)" in hpp and "slideo_group_set_gate_memory(h->g, gate_memory_)" in hpp
    assert "slideo_group_last_gate_refs(h_->g" in hpp and "gate_memory_emission(" in hpp
    assert hpp.index("slideo_group_set_gate_settle(h->g") < hpp.index("slideo_group_set_gate_memory(h->g"), "after the settle"
    from slideo_amd import matching
    assert "gate_memory" in inspect.signature(matching.HipImageVideoMatcher.__init__).parameters
    src = inspect.getsource(matching)
    assert "set_gate_memory(self._gate_memory)" in src and "last_gate_refs()" in src
    assert src.index("set_gate_reference(") < src.index("set_gate_settle(") < src.index("set_gate_memory(")


def test_the_setting_did_not_grow():
    fs = open(os.path.join(ROOT, "slideo_amd", "csrc", "frame_settings.h")).read()
    enum = re.search(r"enum Setting \{(.*?)\}", fs, re.S).group(1)
    names = [n.strip() for n in enum.split(",") if n.strip()]
    assert names[-2:] == ["SET_GATE_REFERENCE", "N_SETTINGS"] and len(names) == 9
    assert "int32_t gate_memory = 0;" in fs


# ---- the restatement on built streams -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pictures(oracle, cfg0_data):
    """Small images of five synthetic frames A .. E and a helper that fades between two of them."""
    _, f, _, _ = cfg0_data
    smalls = gref.small_images(oracle, list(f[:5]))

    def fade(a, b, k):
        a64, b64 = f[a].astype(np.float64), f[b].astype(np.float64)
        return gref.small_images(oracle, [np.rint(a64 + (b64 - a64) * j / k).astype(np.uint8) for j in range(1, k)])

    return smalls, fade


def _holds(smalls, order, length=3):
    return np.stack([smalls[p] for p in order for _ in range(length)])


def test_returns_are_recalled_with_the_right_ordinals(pictures):
    smalls, _ = pictures
    A, B, Cc = 0, 1, 2
    seq = _holds(smalls, [A, B, A, Cc, B])                       # holds A B A C B with hard cuts, three frames each
    ch, sim, kind, refs, state = mref.flags(seq, None, CS, 0, 0, 4)
    assert kind.tolist() == [3, 0, 0, 3, 0, 0, 1, 0, 0, 3, 0, 0, 1, 0, 0], "A and B and C are matched once, the returns are recalled"
    assert refs.tolist() == [0, 0, 0, 3, 3, 3, 0, 0, 0, 9, 9, 9, 3, 3, 3]
    assert [o for _, o in state[0]] == [0, 3, 9] and state[1] == 1 and state[4] == 15, "three entries, the anchor is B's, the next ordinal 15"
    # a recalled frame is changed == 0 && similarity < changed_similarity, like a deferred one; ref tells them apart
    assert (~ch[kind == mref.RECALLED]).all() and (sim[kind == mref.RECALLED] < np.float32(CS)).all()
    # under M = 1 every return is matched, and that is the ANCHOR rule
    ch1, sim1, kind1, refs1, state1 = mref.flags(seq, None, CS, 0, 0, 1)
    assert np.nonzero(ch1)[0].tolist() == [0, 3, 6, 9, 12] and not (kind1 == mref.RECALLED).any()
    ach, asim, _, alast = aref.flags(seq, None, CS)
    assert np.array_equal(ch1, ach) and sim1.tobytes() == asim.tobytes() and np.array_equal(state1[0][state1[1]][0], alast)
    assert refs1.tolist() == [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9, 12, 12, 12]


def test_a_return_to_an_evicted_picture_is_matched_again(pictures):
    smalls, _ = pictures
    A, B, Cc = 0, 1, 2
    seq = _holds(smalls, [A, B, Cc, A, Cc, B], 2)                # M = 2: C evicts A; A again evicts B; C is still there; B is not
    ch, _, kind, refs, state = mref.flags(seq, None, CS, 0, 0, 2)
    assert kind[::2].tolist() == [mref.MATCHED, mref.MATCHED, mref.MATCHED, mref.MATCHED, mref.RECALLED, mref.MATCHED]
    assert refs[::2].tolist() == [0, 2, 4, 6, 4, 10]
    assert [o for _, o in state[0]] == [6, 10], "FIFO: the recall of C (ordinal 4) did not refresh it, B's match dropped it"
    ch4 = mref.flags(seq, None, CS, 0, 0, 4)[0]
    assert int(ch4.sum()) == 3 < int(ch.sum()) == 5


def test_a_fade_back_to_a_remembered_slide_is_recalled_before_it_stands_still(pictures):
    smalls, fade = pictures
    A, B = 0, 1
    seq = np.concatenate([_holds(smalls, [A, B], 4), fade(B, A, 24), _holds(smalls, [A], 4)])
    lo = 8                                                       # the fade's first frame
    ch, sim, kind, refs, state = mref.flags(seq, None, CS, SETTLE, NEVER, 4)
    assert np.nonzero(ch)[0].tolist() == [0, 5], "A on the state none, B on the second frame of its hold; nothing after"
    rec = np.nonzero(kind == mref.RECALLED)[0]
    assert len(rec) == 1 and lo < rec[0] <= lo + 23, "recalled by the fade's end, on a frame that is one step from the frame before it"
    n = seq.shape[1] * seq.shape[2]
    valid = np.ones(seq.shape[1:3], bool)
    assert gref.masked_ssd(seq[rec[0] - 1], seq[rec[0]], valid) >= gref.threshold(SETTLE, n), "the recalled frame is not still"
    assert (kind[lo:rec[0]] == mref.DEFERRED).any() and (refs[kind == mref.DEFERRED] == mref.REF_DEFERRED).all()
    assert (kind[rec[0] + 1:] == mref.UNCHANGED).all() and (refs[rec[0]:] == 0).all()
    # the settle alone matches A a second time, once the picture stands still
    sch = sref.flags(seq, None, CS, SETTLE, NEVER)[0]
    assert int(sch.sum()) == 3 and np.nonzero(sch)[0][-1] >= lo + 23


@pytest.mark.parametrize("settle,max_defer", [(0, 0), (SETTLE, 0), (SETTLE, 4), (SETTLE, NEVER)])
def test_m_1_is_the_rule_without_a_memory(oracle, cfg0_data, settle, max_defer):
    """On tests/test_gate_settle_abi.py's stream: holds, hard cuts, two fades and a noisy hold."""
    _, f, _, _ = cfg0_data
    rng = np.random.default_rng(19)

    def fd(a, b, k):
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        return [a, a, a] + [np.rint(a64 + (b64 - a64) * j / k).astype(np.uint8) for j in range(1, k)] + [b, b, b]

    seq = [f[0]] * 4 + [f[1]] + fd(f[1], f[2], 24) + [f[3]] * 4 + fd(f[4], f[5], 24)
    seq += [np.clip(f[6].astype(np.int16) + rng.integers(-3, 4, f[6].shape), 0, 255).astype(np.uint8) for _ in range(6)]
    smalls = gref.small_images(oracle, seq)
    ch, sim, kind, refs, state = mref.flags(smalls, None, CS, settle, max_defer, 1)
    if settle:
        sch, ssim, skind, _, sstate = sref.flags(smalls, None, CS, settle, max_defer)
        assert np.array_equal(kind == mref.DEFERRED, skind == sref.DEFERRED) and state[3] == sstate[2]
    else:
        sch, ssim, _, last = aref.flags(smalls, None, CS)
        sstate = (last, smalls[-1], 0)
    assert np.array_equal(ch, sch) and sim.tobytes() == ssim.tobytes() and not (kind == mref.RECALLED).any()
    assert np.array_equal(state[0][state[1]][0], sstate[0]) and np.array_equal(state[2], sstate[1])
    # cutting the stream changes nothing
    for cut in (1, 7, 20):
        for M in (1, 3):
            w = mref.flags(smalls, None, CS, settle, max_defer, M)
            a = mref.flags(smalls[:cut], None, CS, settle, max_defer, M)
            b = mref.flags(smalls[cut:], None, CS, settle, max_defer, M, a[4])
            for k in range(4):
                assert np.concatenate([a[k], b[k]]).tobytes() == w[k].tobytes(), (cut, M, k)
            assert [o for _, o in b[4][0]] == [o for _, o in w[4][0]] and b[4][1] == w[4][1] and b[4][3:] == w[4][3:]


def test_the_integer_walk_is_the_rule(pictures):
    """gate_memory_ref.walk over the tables of all pairs = gate_memory_ref.flags over the images: whole stream from "none", and a second
    unit from the ring the first left."""
    smalls, fade = pictures
    seq = np.concatenate([_holds(smalls, [0, 1, 2, 0], 2), fade(0, 3, 8), _holds(smalls, [3, 1, 4, 2, 0], 2)])
    n = seq.shape[1] * seq.shape[2]
    t_c, t_s = gref.threshold(CS, n), gref.threshold(SETTLE, n)
    table = aref.all_pairs_ssd(seq)
    for M, settle, max_defer in ((2, 0, 0), (3, SETTLE, NEVER), (3, SETTLE, 2), (64, 0, 0)):
        ch, sim, kind, refs, state = mref.flags(seq, None, CS, settle, max_defer, M)
        thr_s, cap = (t_s, max_defer) if settle else (0, 0)
        fl, ssd, wrefs, wkind, occ, head, count, anc, d = mref.walk(table, np.zeros((len(seq), M), np.int64), np.zeros(M, np.int64), 0, 0, 0, 0, t_c, thr_s,
                                                                   cap, 0, True, 0, M)
        assert np.array_equal(fl.astype(bool), ch) and np.array_equal(wkind, kind) and np.array_equal(wrefs, refs)
        assert count == len(state[0]) and d == state[3]
        assert sorted(int(o) for o in occ[:M] if o >= 0) == [o for _, o in state[0]]
        cut = 9
        a = mref.flags(seq[:cut], None, CS, settle, max_defer, M)
        E, ai, prev, d0, t0 = a[4]
        # the ring the first unit leaves, entries oldest first from slot 0 (not full) or from head
        cnt = len(E)
        head0 = cnt % M if cnt < M else 1 % M
        slot = [(head0 + k) % M if cnt == M else k for k in range(cnt)]
        ords, mem = np.zeros(M, np.int64), np.zeros((M,) + seq.shape[1:], np.uint8)
        for k, (img, o) in enumerate(E):
            ords[slot[k]], mem[slot[k]] = o, img
        valid = np.ones(seq.shape[1:3], bool)
        mtable = np.array([[gref.masked_ssd(mem[c], s, valid) for c in range(M)] for s in seq[cut:]], np.int64)
        fl, ssd, wrefs, wkind, occ, head, count, anc, d = mref.walk(table[cut:, cut:], mtable, ords, cnt, head0, slot[ai], gref.masked_ssd(prev, seq[cut], valid),
                                                                   t_c, thr_s, cap, d0, False, t0, M)
        assert np.array_equal(fl.astype(bool), ch[cut:]) and np.array_equal(wkind, kind[cut:]) and np.array_equal(wrefs, refs[cut:]), (M, settle, max_defer)
        assert count == len(state[0]) and d == state[3]


# ---- the task's emission --------------------------------------------------------------------------------------------------------------
def test_the_emission_function():
    from slideo_amd import matching
    V = lambda p: {"page_idx": p}
    none = V(-9)
    mem = matching.new_gate_memory(2)
    # call 1: A matched (ordinal 0), held, B matched (3), back to A (recalled, ref 0), held
    changed = [1, 0, 0, 1, 0, 0]
    refs = [0, 0, 0, 3, 0, 0]
    verdicts = [V(5), none, none, V(7), none, none]
    out = matching.gate_memory_emission(changed, refs, verdicts, mem)
    assert [(i, v["page_idx"]) for i, v in out] == [(0, 5), (3, 7), (4, 5)], "the recalled frame emits A's verdict at its own index"
    assert mem["next"] == 6 and mem["prev_ref"] == 0 and sorted(mem["verdicts"]) == [0, 3]
    # call 2: still A (nothing), deferred frames, back to A (emitted again: harmless, the same page), C matched (evicts ordinal 0),
    # B recalled (ordinal 3 survives), a reset's image (ref -1: nothing is known about it)
    changed = [0, 0, 0, 0, 1, 0, 0]
    refs = [0, -2, -2, 0, 10, 3, -1]
    verdicts = [none, none, none, none, V(9), none, none]
    out = matching.gate_memory_emission(changed, refs, verdicts, mem)
    assert [(i, v["page_idx"]) for i, v in out] == [(3, 5), (4, 9), (5, 7)]
    assert sorted(mem["verdicts"]) == [3, 10] and mem["next"] == 13 and mem["prev_ref"] == -1
    # a ref the task no longer remembers emits nothing (it cannot happen with the library's own capacity)
    assert matching.gate_memory_emission([0], [0], [none], mem) == []


# ---- the host check ---------------------------------------------------------------------------------------------------------------------
def _write(f, c):
    fl, ssd, refs, kind, occ, head, count, anc, d = c["want"]
    f.write("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (c["n"], c["M"], c["count"], c["head"], c["anchor"], c["prev_ssd0"], c["thr_c"], c["thr_s"],
                                                      c["max_defer"], c["d_in"], int(c["none"]), c["t0"]))
    for arr in (c["ordinals"], c["table"].reshape(-1), c["mtable"].reshape(-1), fl, ssd, refs, occ):
        f.write(" ".join(str(int(v)) for v in arr) + "\n")
    f.write("%d %d %d %d\n" % (head, count, anc, d))


def test_the_cases_take_every_branch():
    allc = cases.all_stream_cases() + cases.forced_cases()
    kinds = np.concatenate([c["want"][3] for c in allc])
    for k in (mref.UNCHANGED, mref.RECALLED, mref.DEFERRED, mref.MATCHED):
        assert (kinds == k).sum() >= 50, k

    def carried_recall(c):                                       # a recall whose ref is a carried entry's ordinal
        return ((c["want"][3] == mref.RECALLED) & (c["want"][2] < c["t0"])).any()

    def in_unit_recall(c):
        return ((c["want"][3] == mref.RECALLED) & (c["want"][2] >= c["t0"])).any()

    assert sum(map(carried_recall, allc)) >= 20 and sum(map(in_unit_recall, allc)) >= 20
    assert any(int(c["want"][0].sum()) > c["M"] and in_unit_recall(c) for c in allc), "more than M matches in a unit, then a recall"
    assert any(c["d_in"] > 0 and c["want"][3][0] == mref.DEFERRED for c in allc), "a carried count continues"
    forced = {c["what"]: c for c in cases.forced_cases()}
    for what, c in forced.items():
        fl, ssd, refs, kind, occ, head, count, anc, d = c["want"]
        if what.startswith("tie between entries"):
            tied = np.nonzero(kind == mref.RECALLED)[0]
            o = c["ordinals"]
            assert len(tied) >= 1 and c["mtable"][tied[0]][0] == c["mtable"][tied[0]][1] == 0
            assert refs[tied[0]] == max(int(o[s]) for s in range(c["M"]) if c["mtable"][tied[0]][s] == 0), what
        elif what.startswith("best entry at T_c - 1"):
            assert kind[1] == mref.RECALLED and c["mtable"][1].min() == c["thr_c"] - 1, what
        elif what.startswith("best entry at T_c "):
            assert kind[1] == mref.MATCHED and c["mtable"][1].min() == c["thr_c"], what
        elif what.startswith("in-unit eviction"):
            M = c["M"]
            assert fl[:2 * (M + 2):2].all() and kind[2 * (M + 2)] == mref.MATCHED, "picture 0 was evicted: matched again"
            assert kind[2 * (M + 3)] == mref.RECALLED and refs[2 * (M + 3)] == c["t0"] + 2 * (M + 1), "picture M + 1 survives in the unit: recalled"
        elif what.startswith("carried recall"):
            assert kind[2] == mref.RECALLED and refs[2] == 3 and (kind[3:82] == mref.UNCHANGED).all() and (refs[2:82] == 3).all(), what
        elif what.startswith("all deferred"):
            assert (kind == mref.DEFERRED).all() and d == c["n"] + 2, what
        elif what.startswith("none away"):
            assert (kind == mref.UNCHANGED).all() and d == 0, what
    assert len(forced) == 17


def test_host_check_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    allc = [c for c in cases.all_stream_cases() if c["n"] <= 130] + cases.forced_cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("%d\n" % len(allc))
        for c in allc:
            _write(f, c)
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
            os.path.join(ROOT, "tools", "gate_memory_hostcheck.cpp")]
    for tag, extra in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("hostcheck_" + tag))
        subprocess.check_call(base + extra + ["-o", exe])
        out = subprocess.check_output([exe, path]).decode()
        assert "%d walks: as stated" % len(allc) in out, out


def test_the_frame_settings_host_check_still_walks_144_pairs(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "fs_hostcheck")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_settings_hostcheck.cpp"), "-o", exe])
    assert "144 ordered pairs" in subprocess.check_output([exe]).decode()
