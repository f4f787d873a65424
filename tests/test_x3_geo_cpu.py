"""The geometry of the x3 layer kernel (csrc/x3_geo.h: Cfg and its LDS carve, the layer table and its per-layer
record, the tile walk, the staging-unit map), checked against brute force by a stand-alone host program
(tests/x3_geo_check.cpp) for every row of the layer table in every variant the launch code instantiates.  The
program is built and run twice with the host compiler: plain, and with -fsanitize=address,undefined.  It is also
built (host only, no device compile) and run once per A/B table under tools/probes/x3_tables/, so that a change
to the table format or to an assert cannot silently break them."""
import glob
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "uncertaintyquantification_sleepapnea_1dcnn_amd", "csrc")
TABLES = os.path.join(ROOT, "tools", "probes", "x3_tables")


def _build_and_run(exe, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", os.path.join(HERE, "x3_geo_check.cpp"),
           "-o", exe, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_layer_geometry_against_brute_force(tmp_path, sanitize):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    out = _build_and_run(str(tmp_path / "x3_geo_check"), san)
    # 5 layers with and without the per-sample prescale, and the dense-row kernels of blocks 2..5
    assert "14 configurations, 0 failures" in out
    lds = [int(line.rsplit(" ", 2)[1]) for line in out.splitlines() if ": LDS " in line]
    assert len(lds) == 14 and all(0 < b <= 160 * 1024 for b in lds)


def test_probe_tables_still_build_and_hold(tmp_path):
    tables = sorted(glob.glob(os.path.join(TABLES, "*.h")))
    assert len(tables) >= 20, "the A/B tables moved"
    for t in tables:
        out = _build_and_run(str(tmp_path / os.path.basename(t)[:-2]), [f'-DAPNEAUQ_X3_TABLE="{t}"'])
        assert " configurations, 0 failures" in out, t
