"""Speed of the split-conformal evaluation over random patient splits: HIP kernels vs the vectorised torch
formulation on the same GPU and vs the literal golden loop on the CPU.

``python -m bench.conformal_micro [--out profiles/conformal_micro.json]`` times, at R = 1000 splits and 6
miscoverage levels over 16,384 / 131,072 / 1,048,576 windows (about 330 per patient), the per-window means
already on the GPU:

* ``kernel_ms`` (between HIP events, median of ``kernel_runs``): ``prep`` (the sorts and role inputs, once per
  call), ``conformal_select`` with two strata (class-conditional) for pooled and subsample roles and with one
  stratum over the score order (marginal), and ``conformal_count`` at the 12 cuts; all R splits per launch.
* ``wall_ms`` (host clock, median of ``runs`` after a warm-up call): the whole
  ``evaluate_conformal(..., make_plots=False)`` call, patient splits, class-conditional pooled / subsample and
  marginal pooled.
* ``torch_ms``: the same integers (class-conditional, pooled) from torch on the same GPU: the roles of a chunk
  of splits as a (chunk, n) array, four int32 cumulative sums along n, ``searchsorted`` for the ranks and gathers
  at the cuts; checked equal to the kernels' counts, all R splits between HIP events.
* ``golden``: ``split_masks`` + ``golden_conformal_split`` at the 6 levels on the CPU for ``splits_timed`` splits
  (fewer than R); the per-split median and its projection to R splits are recorded, not a measured R-split total.

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

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import conformal as ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import conformal as CF

SEED = 2025
TORCH_WORKSPACE = 1 << 24   # (chunk, n) elements of the torch formulation


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


def torch_counts(pp, seed, n_splits, cal_thr, ppm, n_units):
    """(R, A, 10) int64 counts of the class-conditional pooled evaluation in plain torch, chunks of splits."""
    n, dev = pp["n"], pp["unit"].device
    unit = pp["unit"].long()
    z = (pp["packed"] & 1) != 0
    chunk = max(1, TORCH_WORKSPACE // n)
    units = torch.arange(n_units, device=dev)
    ppm = ppm.long()
    out = []
    for r0 in range(0, n_splits, chunk):
        r = torch.arange(r0, min(n_splits, r0 + chunk), device=dev)[:, None]
        cal = (rng.split_hash(seed, r, units[None, :]) < cal_thr)[:, unit]                   # (chunk, n)
        c0 = torch.cumsum(cal & ~z, 1, dtype=torch.int32)
        c1 = torch.cumsum(cal & z, 1, dtype=torch.int32)
        t0 = torch.cumsum(~cal & ~z, 1, dtype=torch.int32)
        t1 = torch.cumsum(~cal & z, 1, dtype=torch.int32)
        n0, n1 = c0[:, -1:].long(), c1[:, -1:].long()
        k0, k1 = ops.rank_k(n0, ppm[None, :]), ops.rank_k(n1, ppm[None, :])
        m0 = torch.searchsorted(c0, k0.clamp(min=1).to(torch.int32))
        m1 = torch.searchsorted(c1, (n1 - k1 + 1).clamp(min=1).to(torch.int32))
        e0 = torch.where(k0 <= n0, pp["group_end"][m0.clamp(max=n - 1)], torch.full_like(m0, n))
        s1 = torch.where(k1 <= n1, pp["group_start"][m1.clamp(max=n - 1)], torch.zeros_like(m1))
        zero = torch.zeros(len(r), 1, dtype=torch.int32, device=dev)
        cuts = torch.cat([e0, s1], 1)
        tz = torch.stack([torch.gather(torch.cat([zero, t], 1), 1, cuts) for t in (t0, t1)], -1)
        totals = torch.cat([n0, n1, t0[:, -1:].long(), t1[:, -1:].long()], 1)
        out.append(ops.assemble(totals, tz, e0, s1))
    return torch.cat(out)


def measure_size(n, n_splits, alphas, runs, kernel_runs, golden_splits):
    rs = np.random.RandomState(0)
    y = (rs.rand(n) > 0.7).astype(np.int32)
    p = np.clip(rs.rand(n) * 0.6 + 0.25 * y + rs.randn(n) * 0.05, 0.001, 0.999).astype(np.float32)
    pids = np.sort(rs.randint(0, max(2, n // 330), size=n))   # about 330 windows per patient
    pc = torch.from_numpy(p).cuda()
    ppm = torch.as_tensor(ops.alpha_to_ppm(alphas), dtype=torch.int32).cuda()
    half = ops.cal_threshold(0.5)
    out = {"windows": n, "n_splits": n_splits, "levels": len(alphas), "patients": int(len(np.unique(pids)))}

    def dev(mode, cluster):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return CF.evaluate_conformal(pc, y, "bench", alphas=alphas, n_splits=n_splits, patient_ids=pids,
                                         cluster=cluster, mode=mode, random_state=SEED, make_plots=False)

    out["wall_ms"] = {"class_conditional_pooled": _wall(lambda: dev("class_conditional", "pooled"), runs),
                      "class_conditional_subsample": _wall(lambda: dev("class_conditional", "subsample"), runs),
                      "marginal_pooled": _wall(lambda: dev("marginal", "pooled"), runs)}
    res = dev("class_conditional", "pooled")
    out["example"] = {k: res[k] for k in ("coverage_at_0.100", "coverage_at_0.100_ci_lower", "coverage_at_0.100_ci_upper",
                                          "share_singleton_at_0.100", "coverage_violation_rate_at_0.100")}
    pp = CF._prepare(pc, y, pids, "pooled", "class_conditional")
    ps = CF._prepare(pc, y, pids, "subsample", "class_conditional")
    pm = CF._prepare(pc, y, pids, "pooled", "marginal")
    totals, member = ops.select(pp["unit"], pp["packed"], None, None, SEED, 0, n_splits, half, ppm, 2)
    cuts = torch.cat([pp["group_end"][member[:, 0].long().clamp(min=0)],
                      pp["group_start"][member[:, 1].long().clamp(min=0)]], 1).to(torch.int32)
    out["kernel_ms"] = {
        "prep_class_conditional": _events(lambda: CF._prepare(pc, y, pids, "pooled", "class_conditional"), 5),
        "prep_marginal": _events(lambda: CF._prepare(pc, y, pids, "pooled", "marginal"), 5),
        "select_pooled": _events(lambda: ops.select(pp["unit"], pp["packed"], None, None, SEED, 0, n_splits, half, ppm, 2),
                                 kernel_runs),
        "select_subsample": _events(lambda: ops.select(ps["unit"], ps["packed"], ps["within"], ps["ucount"], SEED, 0,
                                                       n_splits, half, ppm, 2), kernel_runs),
        "select_marginal": _events(lambda: ops.select(pm["unit_s"], pm["packed_s"], None, None, SEED, 0, n_splits, half,
                                                      ppm, 1), kernel_runs),
        "count_pooled": _events(lambda: ops.count(pp["unit"], pp["packed"], None, None, SEED, 0, half, cuts), kernel_runs),
        "count_subsample": _events(lambda: ops.count(ps["unit"], ps["packed"], ps["within"], ps["ucount"], SEED, 0, half,
                                                     cuts), kernel_runs),
        "split_counts_pooled": _events(lambda: CF._split_counts(pp, SEED, 0, n_splits, half, ppm, "class_conditional"),
                                       kernel_runs),
    }
    # the torch formulation on the same GPU: equal integers first, then the time
    want = CF._split_counts(pp, SEED, 0, n_splits, half, ppm, "class_conditional")[1]
    assert torch.equal(torch_counts(pp, SEED, n_splits, half, ppm, out["patients"]), want)
    out["torch_ms"] = {"class_conditional_pooled_all_splits": _events(
        lambda: torch_counts(pp, SEED, n_splits, half, ppm, out["patients"]), 3), "chunk_splits": max(1, TORCH_WORKSPACE // n)}
    # the golden loop on the CPU
    ppm_np = ops.alpha_to_ppm(alphas)
    ts = []
    for r in range(golden_splits):
        t0 = time.perf_counter()
        cal, test = CF.split_masks(p, SEED, r, 0.5, pids, "pooled")
        g = [CF.golden_conformal_split(p, y, cal, test, int(a), "class_conditional") for a in ppm_np]
        ts.append((time.perf_counter() - t0) * 1e3)
        assert [g[j]["counts"][c] for j in range(len(ppm_np)) for c in ops.COLS] == want[r].reshape(-1).tolist()
    per = statistics.median(ts)
    out["golden"] = {"splits_timed": len(ts), "ms_per_split_all_levels": round(per, 3),
                     "projected_ms_for_R": round(per * n_splits, 1)}
    out["speedup"] = {
        "kernels_vs_torch": round(out["torch_ms"]["class_conditional_pooled_all_splits"] /
                                  out["kernel_ms"]["split_counts_pooled"], 2),
        "call_vs_golden_projected": round(per * n_splits / out["wall_ms"]["class_conditional_pooled"]["median"], 1)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--n_splits", type=int, default=1000)
    ap.add_argument("--alphas", default="0.01,0.025,0.05,0.1,0.15,0.2")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--golden_splits", default="20,5,2", help="splits of the golden loop timed per size")
    ap.add_argument("--out", default=os.path.join("profiles", "conformal_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("conformal_micro: no GPU; nothing is measured without one")
    _ext.require()
    sizes = [int(v) for v in a.sizes.split(",")]
    gs = [int(v) for v in a.golden_splits.split(",")]
    gs += [gs[-1]] * (len(sizes) - len(gs))
    res = {"bench": "conformal_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "sizes": {}}
    for n, g in zip(sizes, gs):
        res["sizes"][str(n)] = measure_size(n, a.n_splits, [float(v) for v in a.alphas.split(",")], a.runs,
                                            a.kernel_runs, g)
        print(json.dumps({str(n): res["sizes"][str(n)]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
