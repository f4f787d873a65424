"""Speed of the patient-level analysis: the ``patient_reduce`` kernel against a torch formulation on the
same GPU, and the whole ``evaluate_patient_level`` call against the golden NumPy loop.

``python -m bench.patient_micro [--out profiles/patient_micro.json]`` times, at T = 50 passes over 16,384,
131,072 and 1,048,576 windows with about 330 windows per patient and B = 100 replicates:

* ``kernel_ms`` (HIP events, median of ``kernel_runs`` after a warm-up): ``patient_reduce`` with the windows
  grouped by patient and with shuffled codes, each with the achieved GB/s over the bytes it must read (probs,
  the six rows of m it uses, labels, codes); ``torch_counts``, the per-pass positive counts alone as
  ``(probs > 0.5)`` then ``index_add_`` along N on the same GPU (the comparator: it computes ``pass_pos``
  only, not ``rec``); and ``patient_bootstrap`` for all B replicates, parity and hash indices.
* ``wall_ms`` (host clock around work that ends in a device synchronise, median of ``runs`` after a
  warm-up call): the whole ``evaluate_patient_level(..., make_plots=False)`` on predictions that are already
  on the GPU, with parity and with hash indices; and the golden NumPy loop on the same machine's CPU
  (``golden_patient_table``, ``golden_cohort`` and ``golden_cluster_replicates`` with ``golden_boot``
  replicates, which is fewer than B at the largest size, where one replicate takes seconds: the record
  says how many were run, and a speed-up is given only where the golden ran all B).

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
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import patient as P
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import patient_level as PL

from .calib_micro import _events, _wall

SEED = 2025


def synthetic(n, passes, seed=0):
    """Windows grouped by patient (230..430 each), a patient-level prevalence and pass spread."""
    rs = np.random.RandomState(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rs.randint(230, 431)))
    sizes[-1] -= sum(sizes) - n
    if sizes[-1] == 0:
        sizes.pop()
    n_pat = len(sizes)
    code = np.repeat(np.arange(n_pat), sizes).astype(np.int32)
    prevalence, spread = rs.beta(0.7, 1.5, n_pat), rs.uniform(0.3, 3.0, n_pat)
    y = (rs.rand(n) < prevalence[code]).astype(np.int32)
    centre = (np.where(y == 1, 1.5, -1.5) + rs.randn(n)).astype(np.float32)
    probs = np.empty((passes, n), dtype=np.float32)
    for t in range(passes):
        probs[t] = 1.0 / (1.0 + np.exp(-(centre + spread[code].astype(np.float32) * rs.randn(n).astype(np.float32))))
    return probs, y, code, n_pat


def numpy_loop(probs, y, ids, n_boot):
    """The analysis of ``evaluate_patient_level`` in plain float64 NumPy, every replicate recomputed."""
    table = PL.golden_patient_table(probs, y, ids)
    point = PL.golden_cohort(table, probs, y, ids)
    rep = PL.golden_cluster_replicates(table, probs, y, ids, M.parity_bootstrap_indices(len(table), n_boot, SEED))
    ci = {k: (np.nanpercentile([r[k] for r in rep], 2.5), np.nanpercentile([r[k] for r in rep], 97.5)) for k in point}
    return point, ci


def measure_size(n, passes, n_boot, runs, golden_runs, golden_boot, kernel_runs):
    probs, y, code, n_pat = synthetic(n, passes)
    pc, yt, ct = torch.from_numpy(probs).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(code).cuda()
    shuffled = ct[torch.from_numpy(np.random.RandomState(1).permutation(n)).cuda()].contiguous()
    m = uq_ops.metrics(pc)
    out = {"windows": n, "passes": passes, "patients": n_pat, "n_bootstrap": n_boot}
    read_bytes = 4 * n * (passes + 6 + 2)
    kern = {"read_bytes": read_bytes}
    for name, c in (("reduce_grouped", ct), ("reduce_shuffled", shuffled)):
        ms = _events(lambda: P.reduce(pc, m, yt, c, n_pat), kernel_runs)
        kern[name] = {"ms": ms, "gb_per_s": round(read_bytes / ms / 1e6, 1)}
    # the outputs include two zero fills (pass_pos, rec), which the timing above contains
    kern["uq_reduce"] = _events(lambda: uq_ops.metrics(pc), kernel_runs)
    cl, cs = ct.long(), shuffled.long()

    def torch_counts(c):
        return torch.zeros(passes, n_pat, dtype=torch.int32, device="cuda").index_add_(1, c, (pc > 0.5).to(torch.int32))

    assert torch.equal(torch_counts(cl), P.reduce(pc, m, yt, ct, n_pat)[0])
    kern["torch_counts_grouped"] = _events(lambda: torch_counts(cl), kernel_runs)
    kern["torch_counts_shuffled"] = _events(lambda: torch_counts(cs), kernel_runs)
    kern["grouped_vs_torch"] = round(kern["torch_counts_grouped"] / kern["reduce_grouped"]["ms"], 2)
    table = PL.patient_table(pc, y, code)
    prec = torch.from_numpy(table.attrs["patient_record"].array).cuda()
    idx = torch.from_numpy(M.parity_bootstrap_indices(n_pat, n_boot, SEED).astype(np.int32)).cuda()
    kern["bootstrap_parity"] = _events(lambda: P.bootstrap_sums(prec, n_boot, idx=idx), kernel_runs)
    kern["bootstrap_hash"] = _events(lambda: P.bootstrap_sums(prec, n_boot, seed=SEED), kernel_runs)
    out["kernel_ms"] = kern

    def dev(parity):
        return PL.evaluate_patient_level(pc, y, code, "bench", n_bootstrap=n_boot, random_state=SEED, parity=parity,
                                         make_plots=False)

    wall = {"device_parity": _wall(lambda: dev(True), runs), "device_hash": _wall(lambda: dev(False), runs)}
    if golden_runs > 0:
        ts = []
        for _ in range(golden_runs):
            t = time.perf_counter()
            numpy_loop(probs, y, code, golden_boot)
            ts.append((time.perf_counter() - t) * 1e3)
        wall["numpy_golden"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
                                "max": round(max(ts), 3), "runs": golden_runs, "n_bootstrap": golden_boot}
        if golden_boot == n_boot:
            out["speedup_vs_numpy"] = {k: round(wall["numpy_golden"]["median"] / wall[k]["median"], 2)
                                       for k in ("device_parity", "device_hash")}
    out["wall_ms"] = wall
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--golden_runs", default="3,1,1", help="runs of the NumPy loop per size (0: skip it)")
    ap.add_argument("--golden_boot", default="100,100,4", help="replicates of the NumPy loop per size")
    ap.add_argument("--out", default=os.path.join("profiles", "patient_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("patient_micro: no GPU; nothing is measured without one")
    _ext.require()
    sizes = [int(v) for v in a.sizes.split(",")]
    gr = [int(v) for v in a.golden_runs.split(",")]
    gb = [int(v) for v in a.golden_boot.split(",")]
    gr += [gr[-1]] * (len(sizes) - len(gr))
    gb += [gb[-1]] * (len(sizes) - len(gb))
    res = {"bench": "patient_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "sizes": {}}
    for n, g, b in zip(sizes, gr, gb):
        res["sizes"][str(n)] = measure_size(n, a.passes, a.n_bootstrap, a.runs, g, b, a.kernel_runs)
        print(json.dumps({str(n): res["sizes"][str(n)]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
