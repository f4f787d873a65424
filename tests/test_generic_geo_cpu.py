"""The launch geometry of the generic layer-wise path's bf16 and exact-fp32 kernels (csrc/generic_geo.h: their conv
plans, the wgrad row-group planners, the fragment size and the pack grid), checked against brute force by a
stand-alone host program (tests/generic_geo_check.cpp).  The program is built and run twice with
the host compiler: plain, and with -fsanitize=address,undefined."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "uncertaintyquantification_sleepapnea_1dcnn_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_generic_geometry_against_brute_force(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    exe = str(tmp_path / "generic_geo_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                        os.path.join(HERE, "generic_geo_check.cpp"), "-o", exe, *san], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 1_000_000, r.stdout


def test_the_header_builds_alone(tmp_path):
    """Plain C++17 with no HIP header: the host compiler alone, all warnings as errors."""
    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "alone.cpp"
    src.write_text('#include "generic_geo.h"\nint main() { return apneauq::ggeo::kTileRows == 128 ? 0 : 1; }\n')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(tmp_path / "alone")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
