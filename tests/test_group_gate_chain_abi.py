"""The group gate order and the gate state record (include/slideo_amd.h "Group gate order", "Gate state record") on a CPU-only box:
the header declares the sections, the calls and the enumeration, the library exports them at ABI 7, null handles are refused
before the device, the mirrors name the option, and tools/group_gate_chain_hostcheck.cpp — a program with its own main, built with
the host compiler plain, under -fsanitize=address,undefined and under -fsanitize=thread; nothing sanitized is loaded into Python —
walks the rule table of the three set calls, the record header's round trip and refusals, and the baton with real threads."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHER_CALLS = ["slideo_matcher_gate_state_bytes", "slideo_matcher_gate_state_export", "slideo_matcher_gate_state_import"]
GROUP_CALLS = ["slideo_group_set_gate_order", "slideo_group_gate_order", "slideo_group_gate_state_export", "slideo_group_gate_state_import",
               "slideo_group_gate_chain_waited"]
CALLS = MATCHER_CALLS + GROUP_CALLS


def test_header_declares_the_sections_and_the_calls():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    for title in ("---- Gate state record (", "---- Group gate order ("):
        assert title in src, title
    rec = src[src.index("---- Gate state record ("):src.index("---- Group gate order (")]
    for words in ("0x54534753", "eight 32-bit", "little-endian", "3 * sw * sh bytes", "bit for bit", "SLIDEO_ERR_INVALID_ARG",
                  "slideo_matcher_gate_reset(m, NULL, 0, 0)", "idle matcher"):
        assert words in rec, words
    order = src[src.index("---- Group gate order ("):src.index("/* ---- Direct page look-up")]
    for words in ("The N-device group's form", "SLIDEO_GROUP_GATE_HALO", "SLIDEO_GROUP_GATE_CHAIN", "bit for bit", "more members than frames",
                  "whichever of the three set calls", "SLIDEO_ERR_UNSUPPORTED", "never chains", "gate_baton.h", "No kernel reads a peer's memory",
                  "blocks at its first unit"):
        assert words in order, words
    assert re.search(r"#define SLIDEO_GROUP_GATE_HALO\s+0u", src) and re.search(r"#define SLIDEO_GROUP_GATE_CHAIN\s+1u", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name
    assert "#define SLIDEO_ABI_VERSION 7" in src, "additive: the ABI stays 7"
    # the default order keeps the refusals the earlier sections state
    assert "SLIDEO_GATE_ANCHOR is SLIDEO_ERR_UNSUPPORTED" in src


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    assert (capi.GROUP_GATE_HALO, capi.GROUP_GATE_CHAIN) == (0, 1) and capi.GROUP_GATE_ORDERS == {"halo": 0, "chain": 1}
    for cls in (capi.Matcher, capi.Group):
        assert callable(cls.gate_state_export) and callable(cls.gate_state_import)
    assert callable(capi.Group.set_gate_order) and callable(capi.Group.gate_order) and not hasattr(capi.Matcher, "set_gate_order")


def test_null_handles_and_the_binding_refuse_before_the_device(capi):
    L = capi.lib()
    n, o, s = C.c_int64(7), C.c_uint32(7), C.c_double(7.0)
    buf = (C.c_uint8 * 64)()
    assert L.slideo_matcher_gate_state_bytes(None, C.byref(n)) == 1 and n.value == 7
    assert L.slideo_matcher_gate_state_export(None, buf, 64, C.byref(n)) == 1 and n.value == 7
    assert L.slideo_matcher_gate_state_import(None, buf, 32) == 1
    assert L.slideo_group_set_gate_order(None, 1) == 1
    assert L.slideo_group_gate_order(None, C.byref(o)) == 1 and o.value == 7
    assert L.slideo_group_gate_state_export(None, buf, 64, C.byref(n)) == 1 and n.value == 7
    assert L.slideo_group_gate_state_import(None, buf, 32) == 1
    assert L.slideo_group_gate_chain_waited(None, 1, C.byref(s)) == 1 and s.value == 7.0
    obj = capi.Group.__new__(capi.Group)                         # no handle, no device: the binding's own check of the name comes first
    obj._h = C.c_void_p()
    with pytest.raises(capi.SlideoError) as e:
        obj.set_gate_order("ring")
    assert e.value.code == 1
    obj._h = None


def test_mirrors_name_the_option():
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert "pub const SLIDEO_GROUP_GATE_HALO: u32 = 0;" in ffi and "pub const SLIDEO_GROUP_GATE_CHAIN: u32 = 1;" in ffi
    lib = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    assert "pub group_gate_order: u32" in lib and "group_gate_order: ffi::SLIDEO_GROUP_GATE_HALO" in lib and "pub fn group_gate_order(mut self" in lib
    assert "ffi::slideo_group_set_gate_order(h, self.group_gate_order)" in lib
    assert lib.index("ffi::slideo_group_set_gate_order(h") < lib.index("ffi::slideo_group_set_gate_reference(h"), "the order first"
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_group_gate_order(uint32_t order)" in hpp
    assert "slideo_group_set_gate_order(h->g, gate_order_)" in hpp
    assert hpp.index("slideo_group_set_gate_order(h->g") < hpp.index("slideo_group_set_gate_reference(h->g"), "the order first"
    from slideo_amd import matching
    assert "group_gate_order" in inspect.signature(matching.HipImageVideoMatcher.__init__).parameters
    src = inspect.getsource(matching.HipImageVideoMatcher.create_video_matcher)
    assert "set_gate_order(self._group_gate_order)" in src
    assert src.index("set_gate_order(") < src.index("set_gate_reference(") < src.index("set_gate_settle(")


def test_the_setting_enumeration_did_not_grow():
    """The order is the group's own value, not a ninth frame setting of the members."""
    fs = open(os.path.join(ROOT, "slideo_amd", "csrc", "frame_settings.h")).read()
    enum = re.search(r"enum Setting \{(.*?)\}", fs, re.S).group(1)
    names = [n.strip() for n in enum.split(",") if n.strip()]
    assert names[-2:] == ["SET_GATE_REFERENCE", "N_SETTINGS"] and len(names) == 9
    for name in ("gate_record_encode", "gate_record_validate", "group_gate_order_rule", "propose_group_gate_order"):
        assert re.search(r"\binline\b[^\n]*\b%s\(" % name, fs), name
    baton = open(os.path.join(ROOT, "slideo_amd", "csrc", "gate_baton.h")).read()
    assert "hip" not in baton.lower().replace("no hip include", ""), "plain C++"
    for name in ("void publish()", "void fail(", "double await()", "class GateBatonGuard"):
        assert name in baton, name


def test_the_record_layout_in_python(capi):
    """The header the tests parse GPU records with is the one the C++ encodes: 32 bytes, eight little-endian words."""
    head = np.array([0x54534753, 1, 1, 1, 1, 461, 259, 5], "<u4").tobytes()
    assert head[:4] == b"SGST" and len(head) == 32


# ---- the host check ---------------------------------------------------------------------------------------------------------------------
def test_host_check_plain_sanitized_and_under_the_thread_sanitizer(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
            os.path.join(ROOT, "tools", "group_gate_chain_hostcheck.cpp")]
    for tag, extra, part in (("plain", [], "all"), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "all"),
                             ("tsan", ["-fsanitize=thread"], "baton")):
        exe = str(tmp_path / ("hostcheck_" + tag))
        subprocess.check_call(base + extra + ["-o", exe])
        out = subprocess.check_output([exe, part]).decode()
        assert "group gate chain host check (%s): as stated" % part in out, out
        if part == "all":
            assert "rule table: 2016 set calls walked, 384 refused" in out and "record header: 8 round trips" in out, out
        assert "baton: publish / await in both orders, fail, guard, chains of 5 and 8" in out, out


@pytest.mark.parametrize("tool", ["gate_anchor_hostcheck.cpp", "gate_settle_hostcheck.cpp", "frame_settings_hostcheck.cpp"])
def test_the_earlier_host_checks_still_build(tmp_path, tool):
    """They call the two group rules with their old two arguments: the order defaults to HALO, and so do the refusals."""
    cxx = shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "hostcheck")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", tool), "-o", exe])
    if tool == "frame_settings_hostcheck.cpp":
        assert "144 ordered pairs" in subprocess.check_output([exe]).decode()
