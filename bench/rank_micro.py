"""Speed of the rank-statistics analysis (ROC / PR AUC, Mann-Whitney U with bootstrap CIs): HIP kernels vs
the scikit-learn loop and vs the obvious torch formulation on the same GPU.

``python -m bench.rank_micro [--out profiles/rank_micro.json]`` times, at T = 50 passes and B = 100
replicates over 16,384 / 131,072 / 1,048,576 windows, predictions already on the GPU:

* ``kernel_ms`` (between HIP events, median of ``kernel_runs``): ``prep`` (the one sort), ``rank_count`` with
  parity indices and with the counter hash, and ``rank_scan`` (totals + scan + the limit check) for every
  split count G of the sweep and the automatic choice, which is where ``ops.rank.auto_splits`` comes from.
  The rows timed are one chunk of replicates (``ops.rank.chunk_replicates``: all 100 up to 671,088 windows,
  64 at 1,048,576); ``bootstrap_sums`` is the whole B = 100 loop over chunks.
* ``wall_ms`` (host clock, median of ``runs`` after a warm-up call): the whole
  ``evaluate_discrimination(..., make_plots=False)`` call, both tasks, with parity indices (host
  ``RandomState`` draws + upload included), with the counter hash, and with the patient-cluster bootstrap.
* ``golden``: scikit-learn + SciPy on the literal resamples on the same machine's CPU, both tasks,
  ``golden_replicates`` replicates per task (fewer than B where one takes over a second); the per-replicate
  median and its projection to B replicates are recorded, not a measured B-replicate total.
* ``torch_loop_ms``: per replicate ``s[idx]``, ``torch.sort``, cumulative sums and the tie-group ends, in
  float64 on the same GPU, all B replicates of one task between HIP events.

A measurement path that finds no GPU fails.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, rank
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import discrimination as D
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M

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


def torch_replicate(s, z, ix):
    """AUROC, PR AUC and average precision of one literal resample in torch float64: sort, cumulative sums."""
    ss, order = torch.sort(s[ix], descending=True)
    zz = z[ix][order]
    tp, fp = torch.cumsum(zz, 0), torch.cumsum(1.0 - zz, 0)
    end = torch.ones_like(ss, dtype=torch.bool)
    end[:-1] = ss[1:] != ss[:-1]
    tp, fp = tp[end], fp[end]
    p, n = tp[-1], fp[-1]
    zero = torch.zeros(1, dtype=torch.float64, device=s.device)
    tpr, fpr = torch.cat([zero, tp / p]), torch.cat([zero, fp / n])
    auroc = torch.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) * 0.5)
    prec = torch.cat([zero + 1.0, tp / (tp + fp)])
    d_recall = tpr[1:] - tpr[:-1]
    return auroc, torch.sum(d_recall * (prec[1:] + prec[:-1]) * 0.5), torch.sum(d_recall * prec[1:])


def measure_size(n, passes, n_boot, runs, golden_reps, sweep, kernel_runs):
    rs = np.random.RandomState(0)
    y = (rs.rand(n) > 0.7).astype(np.int32)
    probs = np.clip(rs.rand(n)[None] * 0.6 + 0.25 * y[None] + rs.randn(passes, n) * 0.05, 0.001, 0.999).astype(np.float32)
    pids = np.sort(rs.randint(0, max(2, n // 800), size=n))   # about 800 windows per patient
    pc = torch.from_numpy(probs).cuda()
    out = {"windows": n, "passes": passes, "n_bootstrap": n_boot, "patients": int(len(np.unique(pids)))}

    def dev(parity, cluster=False):
        return D.evaluate_discrimination(pc, y, "bench", n_bootstrap=n_boot, random_state=SEED, parity=parity,
                                         patient_ids=pids if cluster else None, make_plots=False)

    out["wall_ms"] = {"device_parity": _wall(lambda: dev(True), runs), "device_hash": _wall(lambda: dev(False), runs),
                      "device_cluster": _wall(lambda: dev(True, True), runs)}
    res = dev(True)
    out["example"] = {k: res[k] for k in ("apnea_auroc", "apnea_auroc_ci_lower", "apnea_auroc_ci_upper", "error_auroc",
                                          "error_auroc_ci_lower", "error_auroc_ci_upper")}
    # kernels alone, task "apnea"
    s, t = D.task_inputs(pc, y, "apnea", device="cuda")
    pr = rank.prep(s, t)
    rows = min(n_boot, rank.chunk_replicates(n))
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, n_boot, SEED).astype(np.int32)).cuda()
    auto = rank.auto_splits(n, rows)
    kern = {"rows": rows, "prep": _events(lambda: rank.prep(s, t), kernel_runs),
            "count_parity": _events(lambda: rank.weights(pr["pos"], n, rows, idx[:rows]), kernel_runs),
            "count_hash": _events(lambda: rank.weights(pr["pos"], n, rows, None, SEED), kernel_runs),
            "auto_splits": auto, "scan": {},
            "bootstrap_sums_parity": _events(lambda: rank.bootstrap_sums(pr, n_boot, idx=idx), kernel_runs),
            "bootstrap_sums_hash": _events(lambda: rank.bootstrap_sums(pr, n_boot, seed=SEED), kernel_runs)}
    w = rank.weights(pr["pos"], n, rows, idx[:rows])
    ref = rank.scan_sums(w, pr["packed"], splits=1)
    for g in sorted(set(sweep) | {auto}):
        bounds = rank.split_bounds(pr["packed"], g)
        assert torch.equal(rank.scan_sums(w, pr["packed"], bounds=bounds), ref)
        kern["scan"][str(g)] = _events(lambda: rank.scan_sums(w, pr["packed"], bounds=bounds), kernel_runs)
    out["kernel_ms"] = kern
    # the torch formulation on the same GPU, one task, all B replicates
    s64, z64 = s.double(), t.double()
    il = idx.long()

    def torch_loop():
        return [torch_replicate(s64, z64, il[b]) for b in range(n_boot)]

    got = torch.stack([v[0] for v in torch_loop()]).cpu().numpy()
    fin = rank.finalize(rank.bootstrap_sums(pr, n_boot, idx=idx))
    assert np.max(np.abs(got - fin["auroc"])) < 1e-9
    out["torch_loop_ms"] = {"one_task_all_replicates": _events(torch_loop, 5)}
    # the golden loop on the CPU: both tasks, a few replicates each
    sc, tc = s.cpu().numpy().astype(np.float64), t.cpu().numpy()
    se, te = (v.cpu().numpy() for v in D.task_inputs(pc, y, "error", device="cuda"))
    hidx = idx[:golden_reps].cpu().numpy()
    ts = []
    for ix in hidx:
        t0 = time.perf_counter()
        D.golden_discrimination(sc[ix], tc[ix])
        D.golden_discrimination(se[ix].astype(np.float64), te[ix])
        ts.append((time.perf_counter() - t0) * 1e3)
    per = statistics.median(ts)
    out["golden"] = {"replicates_timed": len(ts), "ms_per_replicate_both_tasks": round(per, 3),
                     "projected_ms_for_B": round(per * (n_boot + 1), 1)}
    out["speedup_vs_golden_projected"] = {k: round(per * (n_boot + 1) / v["median"], 1) for k, v in out["wall_ms"].items()
                                          if k != "device_cluster"}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--golden_replicates", default="20,5,2", help="replicates of the scikit-learn loop timed per size")
    ap.add_argument("--sweep", default="1,2,4,8,16,32,64")
    ap.add_argument("--out", default=os.path.join("profiles", "rank_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rank_micro: no GPU; nothing is measured without one")
    _ext.require()
    sizes = [int(v) for v in a.sizes.split(",")]
    gr = [int(v) for v in a.golden_replicates.split(",")]
    gr += [gr[-1]] * (len(sizes) - len(gr))
    res = {"bench": "rank_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "workspace_bytes": rank.WORKSPACE_BYTES, "sizes": {}}
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
