"""bench.py driver contract on the CPU: ``--gpus N`` self-launches N ranks (gloo dry run) and the
reported ``n_gpus`` / backend / devices / aggregates match; the UQ aggregates do not depend on the
rank count (masks keyed by global window index, SyncBN over the whole window set)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", *args],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 prints exactly one JSON line
    return json.loads(lines[0])


def test_bench_self_launch_two_ranks_matches_one():
    common = ["--passes", "3", "--members", "2", "--steps", "1", "--warmup", "1", "--no-secondary"]
    two = _bench("--gpus", "2", "--windows", "24", *common)
    one = _bench("--gpus", "1", "--windows", "48", *common)
    assert two["n_gpus"] == 2 and two["backend"] == "gloo" and len(two["devices"]) == 2
    assert one["n_gpus"] == 1
    assert two["config"]["global_batch"] == one["config"]["global_batch"] == 48
    for k in ("mcd_mean_entropy", "de_mean_mutual_info"):
        assert abs(two["extra"][k] - one["extra"][k]) < 1e-5, (k, two["extra"][k], one["extra"][k])
    for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype",
              "data", "config"):
        assert k in two


def test_bench_refuses_world_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--gpus", "2",
                        "--windows", "8", "--passes", "1", "--members", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "refusing" in r.stderr


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A run without ``--full`` meters no collectives, and ``--dump-outputs`` writes the last timed step's
    arrays: float32 / float64, the shapes of T=3 passes, M=2 members, 7 metrics over 16 windows, the same
    bytes from two runs with the same arguments, and aggregate sums that give the result line's figure."""
    import numpy as np

    args = ["--gpus", "1", "--windows", "16", "--passes", "3", "--members", "2", "--steps", "2", "--warmup", "1"]
    a, b = tmp_path / "a", tmp_path / "b"
    out = _bench(*args, "--dump-outputs", str(a))
    _bench(*args, "--dump-outputs", str(b))
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["extra"]["comm"] is None and out["extra"]["fp32_deviation"] is None and out["extra"]["train"] is None
    shapes = {"mcd_probs": (3, 16), "mcd_metrics": (7, 16), "de_probs": (2, 16), "de_metrics": (7, 16),
              "aggregate_sums": (2, 9)}
    assert sorted(os.listdir(a)) == sorted(k + ".npy" for k in shapes)
    for k, shape in shapes.items():
        va, vb = np.load(a / (k + ".npy")), np.load(b / (k + ".npy"))
        assert va.shape == shape and va.dtype in (np.float32, np.float64), (k, va.shape, va.dtype)
        assert va.tobytes() == vb.tobytes(), k
    s = np.load(a / "aggregate_sums.npy")
    assert s[0, 0] == 16 and abs(s[0, 6] / 16 - out["extra"]["mcd_mean_entropy"]) < 1e-6


def test_bench_dump_samples_windows_over_budget(tmp_path):
    """Over the byte budget every per-window array keeps the same seeded sample of the windows."""
    import numpy as np
    import importlib.util

    import torch

    spec = importlib.util.spec_from_file_location("bench_script", os.path.join(ROOT, "bench.py"))  # bench/ is a package
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    outs ={"mcd_probs": torch.rand(3, 40), "mcd_metrics": torch.rand(7, 40), "de_probs": torch.rand(2, 40),
            "de_metrics": torch.rand(7, 40), "aggregate_sums": torch.rand(2, 9, dtype=torch.float64)}
    old = bench.DUMP_BUDGET
    bench.DUMP_BUDGET = 2 * 9 * 8 + 10 * ((3 + 7 + 2 + 7) * 4 + 8)  # room for 10 of the 40 windows
    try:
        bench._dump_outputs(str(tmp_path), outs, 0, 1, seed=5)
        bench._dump_outputs(str(tmp_path / "again"), outs, 0, 1, seed=5)
    finally:
        bench.DUMP_BUDGET = old
    idx = np.load(tmp_path / "window_index.npy")
    assert idx.shape == (10,) and len(set(idx.tolist())) == 10 and (np.diff(idx) > 0).all()
    assert (idx == np.load(tmp_path / "again" / "window_index.npy")).all()
    total = 0
    for k, v in outs.items():
        got = np.load(tmp_path / (k + ".npy"))
        total += got.nbytes
        want = v.numpy() if k == "aggregate_sums" else v.numpy()[:, idx.astype(np.int64)]
        assert (got == want).all(), k
    assert total + idx.nbytes <= 2 * 9 * 8 + 10 * ((3 + 7 + 2 + 7) * 4 + 8)


@pytest.mark.parametrize("n", [1, 3])
def test_launch_spawn_exit_codes(n, tmp_path):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.parallel import launch

    script = tmp_path / "w.py"
    script.write_text("import os, sys\nr = int(os.environ['RANK'])\n"
                      "assert os.environ['WORLD_SIZE'] == '%d' and os.environ['MASTER_ADDR'] == '127.0.0.1'\n"
                      "sys.exit(7 if r == %d - 1 and %d > 1 else 0)\n" % (n, n, n))
    rc = launch.spawn(n, [sys.executable, str(script)])
    assert rc == (7 if n > 1 else 0)


def test_bench_comm_block_counts_collectives():
    """extra.comm: the metered steps after the timed region report, per step and phase,
    how many collectives ran and their bytes.  2 ranks, T=3 passes, M=2 members (member-parallel):
    MC Dropout = one SyncBN all-reduce of (sum, sum of squares) per BN layer and pass, plus one of the
    row count (6 layers x 2 x T); Deep Ensemble = one all_to_all of the member probabilities; then one
    all-reduce of the 2 x 9 fp64 aggregate sums."""
    out = _bench("--gpus", "2", "--windows", "24", "--passes", "3", "--members", "2", "--steps", "1", "--warmup", "1",
                 "--full", "--no-secondary", "--comm-steps", "2")
    c = out["extra"]["comm"]
    assert c["steps"] == 2
    ph = c["phases"]
    chans = 128 + 192 + 224 + 96 + 256 + 96
    assert ph["mcd"]["syncbn_all_reduce"]["count"] == 6 * 2 * 3
    assert ph["mcd"]["syncbn_all_reduce"]["bytes"] == 3 * (chans * 2 * 8 + 6 * 8)
    assert ph["de"]["all_to_all"]["count"] == 1
    assert ph["de"]["all_to_all"]["bytes"] == 2 * 1 * 24 * 4  # (ranks, members per rank, windows per rank) fp32
    assert ph["aggregate"]["all_reduce"]["count"] == 1 and ph["aggregate"]["all_reduce"]["bytes"] == 2 * 9 * 8
    for p in ph.values():
        for v in p.values():
            assert v["ms"] >= 0.0
