"""Speed of the recalibration kernels: ``recal_sums`` / ``recal_apply`` vs the torch float64 formulation of the same
quantities on the same GPU, and the whole fits vs the SciPy golden on the same machine's CPU.

``python -m bench.recal_micro [--out profiles/recal_micro.json]`` times, at T = 50 passes and 8 candidates over
16,384 / 131,072 / 1,048,576 windows of an over-confident synthetic ensemble:

* ``kernel_ms`` (between HIP events, median of ``kernel_runs``, predictions already on the GPU): ``recal_sums`` with
  its range reduction for F = 1 and F = 5 folds and both objectives, and ``recal_apply``;
* ``torch_ms`` (same clock, median of ``torch_runs``): the vectorised float64 formulation of the same sums
  (one ``(T, n)`` pass per candidate; the per-fold sums as F masked sums, a plain sum for one fold) and of the map;
* ``wall_ms`` (host clock around a synchronise, median of ``runs`` after a warm-up call): the whole
  ``fit_recalibration`` and ``cross_recalibrate`` (5 folds by patient) calls, beta / joint;
* ``golden_ms`` (host clock, up to ``golden_max`` windows): ``golden_fit`` (SciPy BFGS on float64 NumPy) on the CPU.

The baselines are the torch formulation and the golden, never the kernel itself.  A measurement path that finds no
GPU fails.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, recal
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops.laplace import labels_u8
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import recalibration as RC

SEED = 2025


def ensemble(n, T, seed=0):
    """True logit N(-1, 1.5), Bernoulli label, member logit 2.5 z + 0.4 + noise; 40 windows per patient."""
    rng = np.random.default_rng(seed)
    z = rng.normal(-1.0, 1.5, n)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.int64)
    logit = 2.5 * z[None] + 0.4 + 0.7 * rng.standard_normal((T, n))
    return (1.0 / (1.0 + np.exp(-logit))).astype(np.float32), y, np.arange(n) // 40


def _wall(fn, runs, sync=True):
    fn()
    ts = []
    for _ in range(runs):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if sync:
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


def torch_sums(p, y, fold, thetas, F, objective):
    """The obvious vectorised float64 formulation on the GPU: (F, Q, 12)."""
    pc = p.double().clamp(1e-7, 1 - 1e-7)
    l1, m0 = torch.log(pc), -torch.log1p(-pc)
    y1 = y == 1
    one = torch.ones_like(l1[0])
    masks = [(fold == f)[:, None] for f in range(F)] if fold is not None else None
    out = []
    for th in thetas:
        u = th[0] * l1 + th[1] * m0 + th[2]
        q, o = torch.sigmoid(u), torch.sigmoid(-u)
        s = q * o
        if objective == "joint":
            hit = torch.where(y1, q.mean(0), o.mean(0))
            r = torch.where(y1, -1.0, 1.0) / hit
            w = s * (o - q)
            gv = [(s * l1).mean(0), (s * m0).mean(0), s.mean(0)]
            G = [(w * l1 * l1).mean(0), (w * l1 * m0).mean(0), (w * l1).mean(0), (w * m0 * m0).mean(0), (w * m0).mean(0),
                 w.mean(0)]
            pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
            cols = [-torch.log(hit)] + [r * v for v in gv] + [r * r * gv[i] * gv[j] + r * G[k]
                                                              for k, (i, j) in enumerate(pairs)]
        else:
            d = q - y1.double()
            cols = [torch.nn.functional.softplus(torch.where(y1, -u, u)).mean(0), (d * l1).mean(0), (d * m0).mean(0),
                    d.mean(0), (s * l1 * l1).mean(0), (s * l1 * m0).mean(0), (s * l1).mean(0), (s * m0 * m0).mean(0),
                    (s * m0).mean(0), s.mean(0)]
        full = torch.stack([one, y1.double()] + cols, dim=1)           # (n, 12)
        # per fold a masked sum: the fastest of the three torch forms tried (a one-hot matmul and index_add_ are slower)
        out.append(torch.stack([(full * m).sum(0) for m in masks]) if masks is not None else full.sum(0, keepdim=True))
    return torch.stack(out, dim=1)


def torch_apply(p, fold, thetas):
    pc = p.double().clamp(1e-7, 1 - 1e-7)
    th = thetas[fold.long()] if fold is not None else thetas[:1].expand(p.shape[1], 3)
    return torch.sigmoid(th[:, 0] * torch.log(pc) - th[:, 1] * torch.log1p(-pc) + th[:, 2]).float()


def measure_size(n, T, Q, a):
    p_h, y_h, pid = ensemble(n, T)
    fold_h = RC.assign_folds(pid, 5, SEED)
    p, y = torch.from_numpy(p_h).cuda(), torch.from_numpy(y_h).cuda()
    y8 = labels_u8(y)
    fold = torch.from_numpy(fold_h).cuda()
    nofold = torch.empty(0, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(1)
    th = torch.from_numpy(np.stack([rng.uniform(0.3, 1.2, Q), rng.uniform(0.3, 1.2, Q), rng.uniform(-0.5, 0.5, Q)], 1)).cuda()
    th5 = th[:5].contiguous()
    rl = recal.range_len(n)
    ops = _ext.ops()
    out = {"windows": n, "T": T, "candidates": Q, "ranges": recal.n_ranges(n), "range_len": rl,
           "lds_bytes": {"F1": recal.lds_bytes(T, 1, Q), "F5": recal.lds_bytes(T, 5, Q)},
           "kernel_ms": {}, "torch_ms": {}, "speedup_vs_torch": {}}
    for F, fd in ((1, None), (5, fold)):
        for obj in ("joint", "member"):
            key = f"sums_F{F}_{obj}"
            fk = nofold if fd is None else fd
            got = ops.recal_sums(p, y8, fk, th, F, recal.OBJECTIVES[obj], rl, 0)
            ref = torch_sums(p, y, fd, th, F, obj)
            assert float(((got - ref).abs() / (ref.abs() + 1e-6 * ref.abs().max())).max()) <= 1e-9, key
            out["kernel_ms"][key] = _events(lambda: ops.recal_sums(p, y8, fk, th, F, recal.OBJECTIVES[obj], rl, 0),
                                            a.kernel_runs)
            out["torch_ms"][key] = _events(lambda: torch_sums(p, y, fd, th, F, obj), a.torch_runs)
    assert float((ops.recal_apply(p, fold, th5) - torch_apply(p, fold, th5)).abs().max()) <= 2.0 ** -23
    out["kernel_ms"]["apply_F5"] = _events(lambda: ops.recal_apply(p, fold, th5), a.kernel_runs)
    out["torch_ms"]["apply_F5"] = _events(lambda: torch_apply(p, fold, th5), a.torch_runs)
    out["speedup_vs_torch"] = {k: round(out["torch_ms"][k] / out["kernel_ms"][k], 2) for k in out["kernel_ms"]}
    # achieved rates of the flagship setting: T n values are read once (4 bytes each); per value and candidate one exp
    tn = T * n
    ms = out["kernel_ms"]["sums_F1_joint"]
    out["rates"] = {"sums_F1_joint_Gvalue_candidates_per_s": round(tn * Q / ms / 1e6, 2),
                    "sums_F1_joint_input_GB_per_s": round(tn * 4 / ms / 1e6, 2),
                    "apply_GB_per_s": round(tn * 8 / out["kernel_ms"]["apply_F5"] / 1e6, 2)}
    fit = RC.fit_recalibration(p, y, "beta", "joint")
    out["wall_ms"] = {"fit_recalibration_beta_joint": _wall(lambda: RC.fit_recalibration(p, y, "beta", "joint"), a.runs),
                      "cross_recalibrate_5_beta_joint": _wall(
                          lambda: RC.cross_recalibrate(p, y, n_folds=5, method="beta", fold=fold_h), a.runs)}
    out["fit_example"] = {"theta": [float(v) for v in fit.theta], "n_iter": fit.n_iter, "nll_before": fit.nll_before,
                          "nll_after": fit.nll_after, "converged": fit.converged}
    if n <= a.golden_max:
        ts = []
        for _ in range(a.golden_runs):
            t = time.perf_counter()
            g = RC.golden_fit(p_h, y_h, "beta", "joint")
            ts.append((time.perf_counter() - t) * 1e3)
        out["golden_ms"] = {"golden_fit_beta_joint": {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
                                                      "max": round(max(ts), 3), "runs": a.golden_runs}}
        out["speedup_vs_golden"] = {"fit": round(out["golden_ms"]["golden_fit_beta_joint"]["median"] /
                                                 out["wall_ms"]["fit_recalibration_beta_joint"]["median"], 1)}
        out["fit_example"]["max_abs_theta_minus_golden"] = float(np.max(np.abs(fit.theta - g["theta"])))
    else:
        out["golden_ms"] = "not measured at this size"
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--torch_runs", type=int, default=20)
    ap.add_argument("--golden_runs", type=int, default=2)
    ap.add_argument("--golden_max", type=int, default=131072, help="largest size the CPU golden is timed at")
    ap.add_argument("--out", default=os.path.join("profiles", "recal_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("recal_micro: no GPU; nothing is measured without one")
    _ext.require()
    res = {"bench": "recal_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "not_measured": ["T other than %d" % a.T, "a one-candidate-per-walk build of recal_sums (the kernel walks "
                            "two candidates at a time)", "occupancy and hardware counters",
                            "golden_fit above %d windows" % a.golden_max],
           "sizes": {}}
    for n in (int(v) for v in a.sizes.split(",")):
        res["sizes"][str(n)] = measure_size(n, a.T, a.candidates, a)
        print(json.dumps({str(n): res["sizes"][str(n)]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()
