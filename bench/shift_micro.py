"""Speed of the shift-corruption kernel (csrc/uq_shift.hip) against its torch float64 emulation on the same GPU.

``python -m bench.shift_micro [--out profiles/shift_micro.json]`` times, at 16,384 / 131,072 / 1,048,576 fp32 windows
of (60, 4) already on the GPU, one launch of K conditions with re-standardisation:

* K = 1 (``gaussian_noise`` at severity 3) and K = 5 (``gaussian_noise``, ``flatline``, ``spikes``, ``clip``,
  ``delay`` at severity 3, all channels);
* ``kernel_ms``: the op between HIP events, median of ``--kernel_runs`` (50) after a warm-up call; ``gb_per_s`` is
  the ``(1 + K) n L C 4`` bytes the algorithm moves (one read of the clean set, K fp32 copies written) over that time;
* ``torch_ms``: ``ops/shift.py:corrupt_eager`` (float64 torch ops, one condition after the other) rounded to fp32,
  on the same GPU between HIP events, median of ``--torch_runs``;
* ``max_err_over_bound``: the largest ``|kernel - emulation| / (2^-23 |emulation| + 1e-12)`` at the timed size
  (at most 1 when the kernel is right) and whether the two agree bitwise after the rounding to fp32;
* ``per_kind_ms`` at 131,072 windows: K = 1 of every kind at severity 3;
* ``same_bytes`` at every size: three K = 5 launches that move the same bytes as ``k5`` with less arithmetic, to tell
  what the kernel's time follows: ``k5_no_restandardize`` (the same five conditions with ``restandardize=False``:
  one set of moments in place of six, no division per element), ``k5_one_channel`` (the five conditions on channel
  0 only: the moments and divisions of a condition for one channel in place of four) and ``k5_copies`` (five times
  severity 0: the clean moments once, then five stores of the same registers).

K other than 1 and 5, fp64 inputs, other window shapes and hardware counters are not measured.  A measurement path
that finds no GPU fails.
"""
import argparse
import json
import os
import statistics

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import shift as S

SEED = 2025
L, C = 60, 4
MIXED = ("gaussian_noise", "flatline", "spikes", "clip", "delay")


def _events(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4), "runs": runs}


def conditions(kinds, severity=3):
    cs = [S.condition(k, severity=severity, C=C) for k in kinds]
    return [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]


def measure(x, conds, kernel_runs, torch_runs, restd=True):
    K, n = len(conds[0]), x.shape[0]
    out = {"K": K, "bytes_moved": (1 + K) * n * L * C * 4}
    out["kernel_ms"] = _events(lambda: S.shift_corrupt(x, *conds, SEED, 0, restd), kernel_runs)
    out["gb_per_s"] = round(out["bytes_moved"] / (out["kernel_ms"]["median"] * 1e-3) / 1e9, 1)
    if torch_runs:
        out["torch_ms"] = _events(lambda: S.corrupt_eager(x, *conds, SEED).float(), torch_runs)
        out["speedup_vs_torch"] = round(out["torch_ms"]["median"] / out["kernel_ms"]["median"], 1)
        got = S.shift_corrupt(x, *conds, SEED)
        worst, same = 0.0, True
        for k in range(K):   # one condition at a time: the float64 emulation of all K at once is large
            ref = S.corrupt_eager(x, [conds[0][k]], [conds[1][k]], [conds[2][k]], SEED)[0]
            worst = max(worst, float(((got[k].double() - ref).abs() / (2.0 ** -23 * ref.abs() + 1e-12)).max()))
            same = same and bool(torch.equal(got[k], ref.float()))
        out["max_err_over_bound"], out["bitwise_equal_after_rounding"] = round(worst, 4), same
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--torch_runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "shift_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("shift_micro: no GPU; nothing is measured without one")
    _ext.require()
    res = {"bench": "shift_micro", "device": torch.cuda.get_device_name(0), "window": [L, C], "dtype": "float32",
           "restandardize": True, "sizes": {}}
    for n in [int(v) for v in a.sizes.split(",")]:
        rs = np.random.RandomState(n % 1000)
        raw = rs.randn(n, L, C) * (rs.rand(1, 1, C) * 50) + rs.randn(n, 1, C) * 10
        x = torch.from_numpy(raw.astype(np.float32)).cuda()
        row = {"windows": n, "k1": measure(x, conditions(MIXED[:1]), a.kernel_runs, a.torch_runs),
               "k5": measure(x, conditions(MIXED), a.kernel_runs, a.torch_runs)}
        k5, one = conditions(MIXED), conditions(MIXED)
        one = (one[0], one[1], [1] * len(MIXED))
        copies = ([S.NONE] * len(MIXED), [0.0] * len(MIXED), [(1 << C) - 1] * len(MIXED))
        row["same_bytes"] = {
            name: {k: v for k, v in measure(x, cd, a.kernel_runs, 0, restd).items() if k in ("kernel_ms", "gb_per_s")}
            for name, cd, restd in (("k5_no_restandardize", k5, False), ("k5_one_channel", one, True),
                                    ("k5_copies", copies, True))}
        if n == 131072:
            row["per_kind_ms"] = {k: measure(x, conditions([k]), a.kernel_runs, 0)["kernel_ms"]["median"]
                                  for k in S.KINDS[1:]}
        res["sizes"][str(n)] = row
        print(json.dumps({str(n): row}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        del x
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
