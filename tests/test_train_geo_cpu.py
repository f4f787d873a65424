"""The launch geometry of the dedicated training path (csrc/train_geo.h: grids, wgrad row groups, partial
slots, reduction shape, deterministic scratch) checked against brute force by a stand-alone host program
(tests/train_geo_check.cpp) built with the host compiler, -Wall -Werror (it also builds and runs clean with
-fsanitize=address,undefined).  The same program's ``--table`` output is where the other tests read the
geometry from (train_kernel_refs.geo)."""
import subprocess

from . import train_kernel_refs as T


def test_train_launch_geometry_against_brute_force():
    r = subprocess.run([T.geo_check_exe()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    # 4202 batch sizes x (1 + 5 member counts x (1 + 6 blocks x 2 modes)), + the 4 literal cases
    assert "277336 cases, 0 failures" in r.stdout


def test_table_output_is_the_launch_of_that_batch():
    g = T.geo(1026)
    assert g["tiles"] == 513 and g["blocks"][1]["fwd"] == {"pf": True, "grid": g["fwd_train_grid"]}
    assert g["blocks"][1]["dgrad"] == {"persist": True, "grid": g["dg_grid"]} and g["blocks"][3]["dgrad"]["grid"] == 513
    assert not T.geo(1026, 1, True)["blocks"][1]["fwd"]["pf"]          # never in deterministic mode
    w = T.wg(5, 37, 3)
    assert w["grid"] == w["nci"] * w["nco"] * w["rgs"] and w["rgs"] * w["rt"] >= T.tiles(37) > (w["rgs"] - 1) * w["rt"]
    assert T.geo(37, 3, True)["blocks"][5]["wgrad"]["rgs"] == T.wg(5, 37, 1)["rgs"]   # deterministic: the M = 1 grouping
