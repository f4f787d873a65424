"""Speed of the pass-count convergence analysis: the ``converge`` kernel, the whole
``evaluate_convergence`` call and the golden NumPy loop.

``python -m bench.convergence_micro [--out profiles/convergence_micro.json]`` times, at T = 50 passes, 101
orders (the identity and 100 random ones), the default counts 1, 2, 3, 5, 10, 15, 20, 30, 40, 50 and 16,384,
131,072 and 1,048,576 windows, with the predictions already on the GPU:

* ``kernel_ms`` (HIP events, median of ``kernel_runs`` after a warm-up): one ``torch.ops.apneauq.converge``
  launch (with the zero fill of its output) at ``rep_groups`` 1, 2, 4 and 8 and at the value that
  ``ops.converge.auto_rep_groups`` picks.  Only the variant that adds with 64-bit integer atomics is
  built; there is no per-workgroup-slot variant to compare it with.
* ``wall_ms`` (host clock around work that ends in a device synchronise, median of ``runs`` after a
  warm-up call): the whole ``evaluate_convergence(..., make_plots=False)`` without files; and the golden
  NumPy loop (``golden_convergence`` and the same percentiles) on the same machine's CPU with
  ``golden_orders`` orders, which is fewer than 101 at the largest size: the record says how many were run,
  and a speed-up is given only where the golden ran all 101.
* ``passes``: the inference passes that one prediction set replaces, ``max(counts)`` against
  ``sum(counts)`` of a sweep that runs every count afresh.  Arithmetic, not a measurement.

A measurement path that finds no GPU fails.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import converge as V
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import convergence as CV

from .calib_micro import _events, _wall

SEED = 2025
REP_GROUPS = (1, 2, 4, 8)


def synthetic(n, passes, seed=0):
    """Every window has its own centre and its own spread of the passes."""
    rs = np.random.RandomState(seed)
    y = (rs.rand(n) < 0.3).astype(np.int32)
    centre = (np.where(y == 1, 1.5, -1.5) + rs.randn(n)).astype(np.float32)
    spread = rs.uniform(0.2, 2.5, size=n).astype(np.float32)
    probs = np.empty((passes, n), dtype=np.float32)
    for t in range(passes):
        probs[t] = 1.0 / (1.0 + np.exp(-(centre + spread * rs.randn(n).astype(np.float32))))
    return probs, y


def numpy_loop(probs, y, counts, n_orders):
    """The curves and bands of ``evaluate_convergence`` in plain float64 NumPy, subset by subset."""
    cur = CV.golden_convergence(probs, y, counts, CV.subset_orders(probs.shape[0], n_orders, SEED))
    return {k: (v[0], v[1:].mean(0), np.percentile(v[1:], 2.5, axis=0), np.percentile(v[1:], 97.5, axis=0))
            for k, v in cur.items()}


def measure_size(n, passes, n_orders, runs, golden_runs, golden_orders, kernel_runs):
    probs, y = synthetic(n, passes)
    pc, yt = torch.from_numpy(probs).cuda(), torch.from_numpy(y).cuda()
    counts = CV.default_counts(passes)
    od = torch.from_numpy(CV.subset_orders(passes, n_orders, SEED)).cuda()
    ct = torch.from_numpy(counts).cuda()
    out = {"windows": n, "passes": passes, "orders": n_orders + 1, "counts": counts.tolist()}
    auto = V.auto_rep_groups(n, n_orders + 1)
    ref = V.sums(pc, yt, od, counts.tolist())
    kern = {"rep_groups": {}, "auto_rep_groups": auto}
    for g in REP_GROUPS:
        assert torch.equal(torch.ops.apneauq.converge(pc, yt, od, ct, g), ref)
        kern["rep_groups"][str(g)] = _events(lambda: torch.ops.apneauq.converge(pc, yt, od, ct, g), kernel_runs)
    kern["auto"] = _events(lambda: torch.ops.apneauq.converge(pc, yt, od, ct, auto), kernel_runs)
    best = min(kern["rep_groups"].values())
    kern["auto_vs_best"] = round(kern["auto"] / best, 3)
    # the work of a launch: a subset's metrics per (window, order, count)
    kern["window_order_counts_per_us"] = round(n * (n_orders + 1) * len(counts) / kern["auto"] / 1e3, 1)
    out["kernel_ms"] = kern

    def dev():
        return CV.evaluate_convergence(pc, y, "bench", n_orders=n_orders, random_state=SEED, output_dir=None,
                                       make_plots=False)

    wall = {"device": _wall(dev, runs)}
    if golden_runs > 0:
        ts = []
        for _ in range(golden_runs):
            t = time.perf_counter()
            numpy_loop(probs, y, counts, golden_orders - 1)
            ts.append((time.perf_counter() - t) * 1e3)
        wall["numpy_golden"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
                                "max": round(max(ts), 3), "runs": golden_runs, "orders": golden_orders}
        if golden_orders == n_orders + 1:
            out["speedup_vs_numpy"] = round(wall["numpy_golden"]["median"] / wall["device"]["median"], 2)
    out["wall_ms"] = wall
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--n_orders", type=int, default=100, help="random orders; the identity is added")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=30)
    ap.add_argument("--golden_runs", default="1,1,1", help="runs of the NumPy loop per size (0: skip it)")
    ap.add_argument("--golden_orders", default="101,101,11", help="orders of the NumPy loop per size, identity included")
    ap.add_argument("--out", default=os.path.join("profiles", "convergence_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("convergence_micro: no GPU; nothing is measured without one")
    _ext.require()
    sizes = [int(v) for v in a.sizes.split(",")]
    gr = [int(v) for v in a.golden_runs.split(",")]
    go = [int(v) for v in a.golden_orders.split(",")]
    gr += [gr[-1]] * (len(sizes) - len(gr))
    go += [go[-1]] * (len(sizes) - len(go))
    counts = CV.default_counts(a.passes)
    res = {"bench": "convergence_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "reduction": "64-bit integer atomics (the only variant built)",
           "passes": {"one_prediction_set": int(counts.max()), "sweep_of_every_count": int(counts.sum()),
                      "reference_counts_5_10_20_30_40_50": {"one_prediction_set": 50, "sweep_of_every_count": 155}},
           "sizes": {}}
    for n, g, o in zip(sizes, gr, go):
        res["sizes"][str(n)] = measure_size(n, a.passes, a.n_orders, a.runs, g, o, a.kernel_runs)
        print(json.dumps({str(n): res["sizes"][str(n)]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
