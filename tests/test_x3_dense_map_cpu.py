"""The dense-row index map shared by the x3 layer kernels and the host bindings (csrc/x3_dense_map.h),
checked against brute force by a stand-alone host program (tests/x3_dense_map_check.cpp) built with the
host compiler (it also builds and runs clean with -fsanitize=address,undefined)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "uncertaintyquantification_sleepapnea_1dcnn_amd", "csrc")

def test_dense_map_against_brute_force(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "x3_dense_map_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{CSRC}", os.path.join(HERE, "x3_dense_map_check.cpp"),
            "-o", exe]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "24 cases, 0 failures" in r.stdout
