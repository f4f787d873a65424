"""Speed of the last-layer Laplace approximation: the two HIP kernels vs the torch float64 formulation on the
same GPU and vs the NumPy golden on the same machine's CPU, and the whole method beside the other two samplers.

``python -m bench.laplace_micro [--out profiles/laplace_micro.json]`` times, at D = 96 and T = 50 over
16,384 / 131,072 / 1,048,576 windows:

* ``kernel_ms`` (between HIP events, median of ``kernel_runs``, features already on the GPU): ``gram``
  (``laplace_gram`` + its range reduction) and ``predict`` (``laplace_predict``, all four outputs);
* ``torch_ms`` (same, the obvious float64 formulation on the same GPU): ``(phi64 * w[:, None]).T @ phi64`` with the
  logits, weights, ``g`` and the log-likelihood, and ``phi64 @ M`` with the sigmoid, the sum of squares and the probit;
* ``golden_ms`` (host clock, median of ``golden_runs``): ``golden_laplace_fit`` / ``golden_laplace_predict``;
* ``wall_ms`` (host clock, median of ``runs`` after a warm-up call, windows already on the GPU): the whole
  ``fit_laplace`` (features + Gram + evidence + factorisation) and ``laplace_predict`` calls on the reference model;
* ``method_ms`` at the first size: ``laplace_predict`` beside ``mc_dropout_predict`` (50 batch-statistics passes) and
  ``deep_ensembles_predict`` (8 members), the headline's two phases.

A measurement path that finds no GPU fails.
"""
import argparse
import json
import math
import os
import statistics
import time

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.cnn import AlarconCNN1D
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import laplace as L
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import laplace as UL
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import uq_techniques as U

SEED = 2025


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


def torch_gram(phi, theta, y):
    """The obvious float64 formulation on the GPU."""
    x = torch.cat([phi.double(), torch.ones(phi.shape[0], 1, dtype=torch.float64, device=phi.device)], dim=1)
    f = x @ theta
    p = torch.sigmoid(f)
    w = p * (1.0 - p)
    H = (x * w[:, None]).T @ x
    g = x.T @ (p - y)
    ll = -torch.nn.functional.softplus(torch.where(y > 0, -f, f)).sum()
    return H, g, ll


def torch_predict(phi, mx, T):
    x = torch.cat([phi.double(), torch.ones(phi.shape[0], 1, dtype=torch.float64, device=phi.device)], dim=1)
    out = x @ mx
    mu = out[:, 0]
    v = (out[:, 1 + T:] ** 2).sum(dim=1)
    return torch.sigmoid(out[:, 1: 1 + T]).T.float().contiguous(), mu, v, torch.sigmoid(mu / torch.sqrt(1.0 + math.pi / 8.0 * v))


def measure_size(n, D, T, model, runs, kernel_runs, golden_runs):
    rs = np.random.default_rng(0)
    phi_h = rs.standard_normal((n, D)).astype(np.float32)
    th_h = rs.standard_normal(D + 1) / math.sqrt(D + 1)
    y_h = (rs.random(n) < 0.3).astype(np.int64)
    phi, th, y = torch.from_numpy(phi_h).cuda(), torch.from_numpy(th_h).cuda(), torch.from_numpy(y_h).cuda()
    y8, yd = L.labels_u8(y), y.double()
    out = {"windows": n, "D": D, "T": T, "ranges": L.n_ranges(n, D), "range_len": L.range_len(n, D),
           "partial_bytes": L.bytes_partial(n, D), "col_blocks": L.col_blocks(D, T)}
    gold = UL.golden_laplace_fit(phi_h, th_h, y_h)
    st = UL.state_from_sums(th_h, gold["H"], gold["g"], gold["loglik"], gold["n_valid"], gold["n_total"], 1.0)
    z = UL.draws(T, D + 1, SEED)
    M = torch.from_numpy(UL.sample_matrix(st, z)).cuda()
    mx = torch.cat([th[:, None], M], dim=1).contiguous()
    rl = L.range_len(n, D)
    ops = _ext.ops()
    flat = ops.laplace_gram(phi, th, y8, rl, 0)
    Ht, gt, _ = torch_gram(phi, th, yd)
    d = L.unflatten(flat, D)
    assert float((d["H"] - Ht).abs().max()) <= 1e-9 * float(Ht.abs().max())
    assert float((d["g"] - gt).abs().max()) <= 1e-9 * max(1.0, float(gt.abs().max()))
    pk = ops.laplace_predict(phi, mx, T)
    pt = torch_predict(phi, mx, T)
    assert float((pk[0] - pt[0]).abs().max()) <= 2.0 ** -22 and float((pk[1][1] - pt[2]).abs().max()) <= 1e-9
    out["kernel_ms"] = {"gram": _events(lambda: ops.laplace_gram(phi, th, y8, rl, 0), kernel_runs),
                        "predict": _events(lambda: ops.laplace_predict(phi, mx, T), kernel_runs)}
    out["torch_ms"] = {"gram": _events(lambda: torch_gram(phi, th, yd), kernel_runs),
                       "predict": _events(lambda: torch_predict(phi, mx, T), kernel_runs)}
    out["golden_ms"] = {"fit": _wall(lambda: UL.golden_laplace_fit(phi_h, th_h, y_h), golden_runs, sync=False),
                        "predict": _wall(lambda: UL.golden_laplace_predict(phi_h, st, T, SEED), golden_runs, sync=False)}
    out["speedup_vs_torch"] = {k: round(out["torch_ms"][k] / out["kernel_ms"][k], 2) for k in ("gram", "predict")}
    out["speedup_vs_golden"] = {"gram": round(out["golden_ms"]["fit"]["median"] / out["kernel_ms"]["gram"], 1),
                                "predict": round(out["golden_ms"]["predict"]["median"] / out["kernel_ms"]["predict"], 1)}
    # whole calls on the reference model, windows on the GPU
    x = torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(1)).cuda()
    fit_state = UL.fit_laplace(model, x, y_h, prior_precision="auto")
    out["wall_ms"] = {"fit_laplace": _wall(lambda: UL.fit_laplace(model, x, y_h, prior_precision="auto"), runs),
                      "laplace_predict": _wall(lambda: UL.laplace_predict(model, fit_state, x, T, SEED, as_numpy=False,
                                                                          return_moments=True), runs),
                      "features_only": _wall(lambda: model.last_layer_features(x), runs)}
    out["fit_example"] = {k: v for k, v in fit_state.scalars().items()}
    return out, x


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--D", type=int, default=SPEC.final_channels)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--golden_runs", type=int, default=3)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "laplace_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("laplace_micro: no GPU; nothing is measured without one")
    _ext.require()
    if a.D != SPEC.final_channels:
        raise SystemExit("the whole-call rows run the reference model: D must be its final channel count")
    sizes = [int(v) for v in a.sizes.split(",")]
    model = AlarconCNN1D(spec=SPEC, params=R.synthetic_params(SPEC, 5), device="cuda")
    res = {"bench": "laplace_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "sizes": {}}
    first_x = None
    for n in sizes:
        res["sizes"][str(n)], x = measure_size(n, a.D, a.T, model, a.runs, a.kernel_runs, a.golden_runs)
        if first_x is None:
            first_x = x
        del x
        print(json.dumps({str(n): res["sizes"][str(n)]}), flush=True)
    # the whole method beside the headline's two phases, first size
    n0 = first_x.shape[0]
    st = UL.fit_laplace(model, first_x, (np.arange(n0) % 3 == 0).astype(np.int64))
    members = [AlarconCNN1D(spec=SPEC, params=R.synthetic_params(SPEC, 100 + m), device="cuda") for m in range(a.members)]
    res["method_ms"] = {
        "windows": n0,
        "laplace_predict_T50": _wall(lambda: U.laplace_predict(model, st, first_x, a.T, SEED, as_numpy=False), a.runs),
        "mc_dropout_batch_bn_T50": _wall(lambda: U.mc_dropout_predict(model, first_x, 50, bn_mode="batch", seed=SEED,
                                                                      as_numpy=False), 5),
        "deep_ensemble_8": _wall(lambda: U.deep_ensembles_predict(members, first_x, as_numpy=False), 5),
    }
    print(json.dumps({"method_ms": res["method_ms"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()
