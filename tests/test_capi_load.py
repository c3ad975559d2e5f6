"""The C-ABI library loads on a CPU-only box and exports every symbol that
include/slideo_amd.h declares; compute calls fail loudly without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(slideo_[a-z0-9_]+)\s*\(", src)) - {"slideo_progress_fn"})


def test_library_exports_every_declared_symbol(capi):
    L = capi.lib()
    names = _declared_symbols()
    assert len(names) >= 19
    for n in names:
        assert hasattr(L, n), "missing export " + n
    assert sorted(capi.EXPORTS) == names
    assert L.slideo_abi_version() == 7        # ABI 7: + slideo_matcher_read_shader_clock (6: verdict_rule, slideo_device_list, n_devices 0; ocv.hdlt defaults to 1)


def test_header_lists_every_environment_switch():
    """include/slideo_amd.h "Environment" lists every SLIDEO_* variable that csrc/ reads, and csrc/ reads every one listed there
    (the build-time line aside: the Python build and loader read those)."""
    hdr = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    block = hdr[hdr.index(" * Environment"):]
    block = block[:block.index("*/")]
    listed = {n for line in block.splitlines() if "build time only" not in line for n in re.findall(r"\bSLIDEO_[A-Z0-9_]+", line)}
    csrc = os.path.join(ROOT, "slideo_amd", "csrc")
    read = set()
    for f in os.listdir(csrc):
        read |= set(re.findall(r'(?:env_long|getenv)\("(SLIDEO_[A-Z0-9_]+)"', open(os.path.join(csrc, f)).read()))
    assert len(read) >= 10
    assert not read - listed, "read in csrc/ but not listed in the header: %s" % sorted(read - listed)
    assert not listed - read, "listed in the header but read nowhere in csrc/: %s" % sorted(listed - read)


def test_config_struct_matches_oracle_layout(capi, oracle):
    import ctypes as C
    a, b = capi.default_config(), oracle.default_config()
    assert C.sizeof(a) == C.sizeof(b) == 168        # ABI 6: + verdict_rule (160 since ABI 4: verify_model, matcher, lsh_*, ocv.hdlt)
    assert bytes(a) == bytes(b)


def test_unsupported_config_is_rejected(capi):
    from conftest import HAS_GPU
    with pytest.raises(capi.SlideoError) as e:
        capi.Matcher(capi.default_config(patch_size=31))
    assert e.value.code in (5,)      # UNSUPPORTED is checked before the device probe


def test_no_silent_cpu_fallback(capi):
    from conftest import HAS_GPU
    if HAS_GPU:
        pytest.skip("GPU present")
    with pytest.raises(capi.SlideoError) as e:
        capi.Matcher()
    assert e.value.code == 2          # SLIDEO_ERR_NO_DEVICE


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "slideo_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                txt = open(os.path.join(d, f), errors="ignore").read()
                assert "pyoracle" not in txt and "liboracle" not in txt and "slideo_oracle" not in txt, f


def test_search_kernel_issues_the_unscaled_matrix_instruction():
    """The exact-Hamming search (csrc/knn_tile.hip.h, KtHamming::mfma) is built on v_mfma_f32_32x32x64_f8f6f4 — the 64-bit encoding the
    compiler selects when both scale operands of the builtin are the constant 0 — not on the 128-bit v_mfma_scale_… double instruction
    (round 6, experiment 10: bit-identical, 2-3 % faster).  Read from the gfx950 code object of the built stage unit, no GPU needed."""
    import re
    import shutil
    import subprocess
    import tempfile
    objdump, objcopy = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-objcopy"
    obj = os.path.join(ROOT, "slideo_amd", "lib", "obj", "stage_knn.o")
    if not (os.path.exists(objdump) and os.path.exists(objcopy) and os.path.exists(obj)):
        pytest.skip("no llvm-objdump / built stage object here")
    tmp = tempfile.mkdtemp()
    try:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
        blob = open(fat, "rb").read()
        elf = os.path.join(tmp, "co.elf")
        open(elf, "wb").write(blob[blob.find(b"\x7fELF"):])
        asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", elf], capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # the kernels of the Hamming engine: every FP4 matrix instruction in the unit
    plain = len(re.findall(r"\bv_mfma_f32_32x32x64_f8f6f4\b", asm))
    scaled = len(re.findall(r"\bv_mfma_scale_f32_32x32x64_f8f6f4\b", asm))
    assert plain > 0 and scaled == 0, (plain, scaled)
