"""The host half of a decode launch (LaunchLayout, launch_errors, tiff_codec_check in
csrc/source_plan.cpp) needs no device: scripts/launch_layout_san.cpp, which checks it against
numbers and messages written out by hand, is compiled and linked with that unit alone by plain
g++ -- no hipcc, no ROCm include path, no sanitizer -- and passes.  (`make san` runs it under
AddressSanitizer / UBSan with the other stand-alone programs.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_launch_layout_builds_and_runs_without_hip(tmp_path):
    exe = str(tmp_path / "launch_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "omero-ms-pixel-buffer_amd", "csrc", "source_plan.cpp"),
                           os.path.join(ROOT, "scripts", "launch_layout_san.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.strip().splitlines()[-1] == "all as expected", out.stdout
