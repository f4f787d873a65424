"""The XCD-aware workgroup order every kernel shares (csrc/xcd_order.h) and the slot geometry shared by the
two fused tiled kernels (csrc/fused_tiled_geo.h), checked against brute force by a stand-alone host program
(tests/tiled_geo_check.cpp) built with the host compiler (it also builds and runs clean with
-fsanitize=address,undefined)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "uncertaintyquantification_sleepapnea_1dcnn_amd", "csrc")

def test_tiled_geometry_and_xcd_order_against_brute_force(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tiled_geo_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{CSRC}", os.path.join(HERE, "tiled_geo_check.cpp"),
            "-o", exe]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 300 grid sizes x 4 XCD counts, + 4 (net, precision) types x 6 blocks
    assert "1224 cases, 0 failures" in r.stdout
