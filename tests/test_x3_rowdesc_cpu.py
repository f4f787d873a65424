"""The per-tile row descriptors of the x3 layer kernels (csrc/x3_dense_map.h: desc_pack, row_desc,
slot_row_desc, mask_word), checked against brute force by a stand-alone host program
(tests/x3_rowdesc_check.cpp) for every tile offset (0, 4, .., 56), both tile sizes and PAD 1..4.  The
program is built and run twice with the host compiler: plain, and with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "uncertaintyquantification_sleepapnea_1dcnn_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_row_descriptors_against_brute_force(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "x3_rowdesc_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{CSRC}", os.path.join(HERE, "x3_rowdesc_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "120 tile cases, 0 failures" in r.stdout
