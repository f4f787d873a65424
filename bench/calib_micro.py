"""Speed of the calibration / selective-prediction analysis: HIP kernels vs the golden NumPy loop.

``python -m bench.calib_micro [--out profiles/calib_micro.json]`` times, at T = 50 passes over 16,384 and
over 1,048,576 windows with B = 100 replicates, K = 15 bins and 11 coverages:

* ``wall_ms``: the whole ``evaluate_calibration(..., make_plots=False)`` call on predictions that are
  already on the GPU, with parity indices (host ``RandomState`` draws + upload included) and with the
  device counter hash; and the golden NumPy loop (``uq/calibration.py golden_*``: per-window metrics,
  thresholds, point values, B full recomputations, percentiles) on the same machine's CPU.  Host
  clock around work that ends in a device synchronise; median over ``runs`` after a warm-up call.
* ``kernel_ms``: ``calib_prep`` and ``calib_bootstrap`` alone between HIP events, the latter for every
  slice count G of the sweep (median of ``kernel_runs``), which is where ``ops.calib.auto_slices`` comes from.

A measurement path that finds no GPU fails.
"""
import argparse
import json
import os
import statistics
import time
import warnings

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, calib
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M

K = 15
COVERAGES = np.linspace(0.5, 1.0, 11)
SEED = 2025


def _wall(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "runs": runs}


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
    return round(statistics.median(ts), 4)


def numpy_loop(probs, y, n_boot):
    """The analysis of ``evaluate_calibration`` in plain float64 NumPy, every replicate recomputed."""
    w = M.per_window(probs)
    p, s = w["mean_pred"].astype(np.float64), w["total_pred_entropy"]
    thr = C.coverage_thresholds(s, COVERAGES)
    pt = {**C.golden_calibration(p, y, K), **C.golden_selective(p, s, y, thr)}
    rep = C.golden_replicates(p, s, y, thr, M.parity_bootstrap_indices(len(y), n_boot, SEED), K)
    with warnings.catch_warnings():  # empty bins are NaN in every replicate
        warnings.simplefilter("ignore", category=RuntimeWarning)
        ci = {k: (np.nanmean(v, axis=0), np.nanpercentile(v, 2.5, axis=0), np.nanpercentile(v, 97.5, axis=0))
              for k, v in rep.items() if k != "bin_count"}
    return pt, ci


def measure_size(n, passes, n_boot, runs, golden_runs, sweep, kernel_runs=50):
    rs = np.random.RandomState(0)
    probs = np.clip(rs.rand(n)[None] * 0.8 + 0.1 + rs.randn(passes, n) * 0.05, 0.001, 0.999).astype(np.float32)
    y = (rs.rand(n) < probs.mean(0)).astype(np.int32)
    pc = torch.from_numpy(probs).cuda()
    out = {"windows": n, "passes": passes, "n_bootstrap": n_boot, "n_bins": K, "coverages": len(COVERAGES)}

    def dev(parity):
        return C.evaluate_calibration(pc, y, "bench", n_bootstrap=n_boot, random_state=SEED, parity=parity, n_bins=K,
                                      coverages=COVERAGES, make_plots=False)

    wall = {"device_parity": _wall(lambda: dev(True), runs), "device_hash": _wall(lambda: dev(False), runs)}
    ts = []
    for _ in range(golden_runs):
        t = time.perf_counter()
        numpy_loop(probs, y, n_boot)
        ts.append((time.perf_counter() - t) * 1e3)
    wall["numpy_golden"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
                            "max": round(max(ts), 3), "runs": golden_runs}
    out["wall_ms"] = wall
    out["speedup_vs_numpy"] = {k: round(wall["numpy_golden"]["median"] / wall[k]["median"], 2)
                               for k in ("device_parity", "device_hash")}
    # kernels alone
    mt = uq_ops.metrics(pc)
    p, s = mt[uq_ops.MEAN].contiguous(), mt[uq_ops.ENT_NATS].contiguous()
    yt = torch.from_numpy(y).cuda()
    thr = torch.from_numpy(C.coverage_thresholds(s, COVERAGES)).cuda()
    j = thr.numel()
    rec = calib.prep(p, s, yt, thr, K)
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, n_boot, SEED).astype(np.int32)).cuda()
    auto = calib.auto_slices(n, n_boot)
    kern = {"prep": _events(lambda: calib.prep(p, s, yt, thr, K), kernel_runs), "auto_slices": auto,
            "bootstrap_parity": {}, "bootstrap_hash": {}}
    ref = calib.bootstrap_sums(rec, n_boot, K, j, idx=idx, slices=1)
    ref_h = calib.bootstrap_sums(rec, n_boot, K, j, seed=SEED, slices=1)
    for g in sorted(set(sweep) | {auto}):
        assert torch.equal(calib.bootstrap_sums(rec, n_boot, K, j, idx=idx, slices=g), ref)
        assert torch.equal(calib.bootstrap_sums(rec, n_boot, K, j, seed=SEED, slices=g), ref_h)
        kern["bootstrap_parity"][str(g)] = _events(lambda: calib.bootstrap_sums(rec, n_boot, K, j, idx=idx, slices=g), kernel_runs)
        kern["bootstrap_hash"][str(g)] = _events(lambda: calib.bootstrap_sums(rec, n_boot, K, j, seed=SEED, slices=g), kernel_runs)
    out["kernel_ms"] = kern
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,1048576")
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50, help="runs per HIP-event kernel timing (tens of microseconds each)")
    ap.add_argument("--golden_runs", default="10,3", help="runs of the NumPy loop per size (it takes minutes at 2^20 windows)")
    ap.add_argument("--sweep", default="1,2,3,4,8,16,32")
    ap.add_argument("--out", default=os.path.join("profiles", "calib_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("calib_micro: no GPU; nothing is measured without one")
    _ext.require()
    sizes = [int(v) for v in a.sizes.split(",")]
    gr = [int(v) for v in a.golden_runs.split(",")]
    gr += [gr[-1]] * (len(sizes) - len(gr))
    res = {"bench": "calib_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "sizes": {}}
    for n, g in zip(sizes, gr):
        res["sizes"][str(n)] = measure_size(n, a.passes, a.n_bootstrap, a.runs, g, [int(v) for v in a.sweep.split(",")],
                                            a.kernel_runs)
        print(json.dumps({str(n): res["sizes"][str(n)]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
