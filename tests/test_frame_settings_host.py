"""The rules of csrc/frame_settings.h on the host: tools/frame_settings_hostcheck.cpp (its own main, no GPU, nothing loaded into
Python) built with the host compiler and run.  The program holds the tables it asserts against; its header names the sanitizer
build, which is run by hand on a CPU machine."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_of_the_frame_settings_rules(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "hostcheck")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_settings_hostcheck.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert "144 ordered pairs" in out, out
