"""The YUV door's argument builder, pinned: which wide loads and stores it chooses for a layout at an address.

tests/golden/yuv_args_flags.txt holds what the four tools/yuv_*_hostcheck.cpp programs printed for a fixed list of cases when every
kernel family still had an argument builder of its own.  This replays the list through today's programs and asserts that every
case prints the same numbers: it fails at any commit where one case's flags move (the *_abi tests assert only that every value is
seen somewhere).

The cases, per family: every sampling / depth pair the family has, every format, the layouts of the family's reference module
(layouts()) at 18x10 and 66x34, one frame and two, the source 0, 2, 4 and 8 bytes past a 16-byte aligned base; and each family's
"pitched" layout, whose rows allow every wide load, once more with the frames 2 bytes further apart than they need be
("pitched+2": a frame stride of 2 mod 4, which alone must take the wide loads away — for the 4:2:0 description kernel under one
frame too, for the others under two).
  desc, sampling   one run per offset; the program prints "wide_y A wide_c B out4 C": the line holds A B C per offset
  chroma, transfer the program itself walks offsets 0, 1, 2, 4 and 8 and prints how often each load and store path was taken, summed
                   over the five: the line holds those counts (the record count left out), which move with any offset's flags
The frames are zeros: the flags depend on addresses alone.

    python tests/test_yuv_args_golden.py [<source root>]     rewrites the fixture from the programs as they are, or as they are in
                                                             another checkout (only when a rule changes on purpose)
"""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yuv_args_flags.txt")
SIZES = ((18, 10), (66, 34))
OFFSETS = (0, 2, 4, 8)


def _build(tmp, family, root):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = os.path.join(tmp, family)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "slideo_amd", "csrc"),
                           os.path.join(root, "tools", "yuv_%s_hostcheck.cpp" % family), "-o", exe])
    return exe


def _numbers(text):
    return " ".join(text.split()[1::2])


def _run(exe, tmp, header, payload):
    cin = os.path.join(tmp, "case.bin")
    with open(cin, "wb") as f:
        f.write(header)
        f.write(bytes(payload))
    return subprocess.check_output([exe, "convert", cin, os.path.join(tmp, "out.bin")]).decode()


def _lay(L, fb):
    return (L.y_stride, L.uv_stride, L.uv_step), (L.u_offset, L.v_offset, fb)


def _with_stride_2_mod_4(layouts):
    """The layouts, and the pitched one again with a frame stride 2 bytes longer."""
    out = list(layouts)
    name, L, fb = next(l for l in out if l[0] == "pitched")
    assert fb % 4 == 0
    return out + [("pitched+2", L, fb + 2)]


def cases(capi, tmp, root=ROOT):
    """Yields (key, numbers) in a fixed order."""
    import yuv_chroma_ref as CR
    import yuv_desc_ref as D
    import yuv_sampling_ref as S
    import yuv_transfer_ref as T

    exe = {f: _build(tmp, f, root) for f in ("desc", "sampling", "chroma", "transfer")}
    for w, h in SIZES:
        for n in (1, 2):
            size = "%dx%d n%d" % (w, h, n)
            for depth in D.DEPTHS:
                for fmt in D.FORMATS:
                    for name, L, fb in _with_stride_2_mod_4(D.layouts(capi, fmt, w, h, depth)):
                        i3, q3 = _lay(L, fb)
                        got = [_numbers(_run(exe["desc"], tmp, struct.pack("<10i3q", w, h, n, 1, 0, depth, *i3, ofs, *q3), n * fb)) for ofs in OFFSETS]
                        yield "desc 0 %d %s %s %s" % (depth, fmt, name, size), " | ".join(got)
            for s in S.SAMPLINGS:
                for depth in S.DEPTHS[s]:
                    for fmt in S.FORMATS[s]:
                        for name, L, fb in _with_stride_2_mod_4(S.layouts(capi, fmt, w, h, depth)):
                            i3, q3 = _lay(L, fb)
                            got = [_numbers(_run(exe["sampling"], tmp, struct.pack("<12i3q", w, h, n, 1, 0, depth, s, *i3, ofs, 0, *q3), n * fb))
                                   for ofs in OFFSETS]
                            yield "sampling %d %d %s %s %s" % (s, depth, fmt, name, size), " | ".join(got)
            for s in CR.SAMPLINGS:
                for depth in CR.DEPTHS[s]:
                    for fmt in CR.FORMATS[s]:
                        for name, L, fb in _with_stride_2_mod_4(CR.layouts(capi, fmt, w, h, depth)):
                            i3, q3 = _lay(L, fb)
                            text = _run(exe["chroma"], tmp, struct.pack("<12i3q", w, h, n, 1, 0, depth, s, *i3, CR.CENTER, n * fb, *q3), n * fb)
                            yield "chroma %d %d %s %s %s" % (s, depth, fmt, name, size), " ".join(text.split()[3::2])
            for s in T.SAMPLINGS:
                for depth in T.DEPTHS:
                    for fmt in T.FORMATS[s]:
                        for name, L, fb in _with_stride_2_mod_4(T.layouts(capi, fmt, w, h, depth)):
                            i3, q3 = _lay(L, fb)
                            text = _run(exe["transfer"], tmp, struct.pack("<12i3q", w, h, n, T.HLG, 0, depth, s, *i3, 0, n * fb, *q3), n * fb)
                            yield "transfer %d %d %s %s %s" % (s, depth, fmt, name, size), " ".join(text.split()[3::2])


def test_every_case_prints_the_recorded_flags(capi, tmp_path):
    want = [l.rstrip("\n").split(" : ") for l in open(GOLDEN) if l.strip()]
    got = [[k, v] for k, v in cases(capi, str(tmp_path))]
    assert [k for k, _ in got] == [k for k, _ in want], "the list of cases itself changed"
    moved = [(k, w, g) for (k, w), (_, g) in zip(want, got) if w != g]
    assert not moved, "%d of %d cases: first (case, recorded, now) %s" % (len(moved), len(want), moved[:3])
    for family in ("desc", "sampling", "chroma", "transfer"):
        assert sum(k.startswith(family + " ") for k, _ in want) >= 48, family


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from slideo_amd import _capi
    with tempfile.TemporaryDirectory() as tmp:
        lines = ["%s : %s\n" % kv for kv in cases(_capi, tmp, *sys.argv[1:2])]
    open(GOLDEN, "w").write("".join(lines))
    print("%d cases -> %s" % (len(lines), GOLDEN))
