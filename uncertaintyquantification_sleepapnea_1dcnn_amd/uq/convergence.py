"""How many MC-Dropout passes, or ensemble members, are enough: convergence curves from one prediction set.

Both samplers return the whole ``(T, N)`` array of probabilities.  The first k passes of one ordering are a
k-subset, and the first k entries of a random permutation are a uniformly random k-subset, so one read of
the array gives the metrics at every count, and R permutations give the expected curve and its spread:
"would 8 of my 20 members have given the same uncertainty?" is answered from the 20 members' predictions,
without another inference run.  :func:`convergence_curves` returns the ``(R, K)`` curves,
:func:`evaluate_convergence` the flat dictionary with percentile bands and the count from which each metric
stays within a tolerance of its all-T value.  The sums behind them come from ``ops/converge.py``
(``csrc/uq_converge.hip`` on CUDA predictions, the eager emulation otherwise).

:func:`golden_convergence` is plain float64 NumPy, subset by subset from the raw probabilities (no
quantisation, two-pass variance): the test oracle and the timing baseline.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd

from . import calibration as C
from . import metrics as M

plt = C.plt

METRICS = M.AGG_KEYS + ("accuracy", "flip_rate", "mean_abs_shift")
DEFAULT_COUNTS = (1, 2, 3, 5, 10, 15, 20) + tuple(range(30, 130, 10))


def _torch():
    import torch

    return torch


def subset_orders(t_count: int, n_orders: int, random_state: Optional[int]) -> np.ndarray:
    """(n_orders + 1, T) int32: row 0 is the identity, the passes as they were run; rows 1.. are successive
    ``np.random.RandomState(random_state).permutation(T)`` draws.  Always drawn on the host."""
    if t_count < 1 or n_orders < 0:
        raise ValueError("t_count >= 1 and n_orders >= 0")
    rs = np.random.RandomState(random_state)
    rows = [np.arange(t_count)] + [rs.permutation(t_count) for _ in range(n_orders)]
    return np.stack(rows).astype(np.int32)


def default_counts(t_count: int, counts: Optional[Sequence[int]] = None) -> np.ndarray:
    """Sorted unique counts clipped to 1..T, with T appended when absent."""
    c = np.asarray(DEFAULT_COUNTS if counts is None else counts, dtype=np.int64).reshape(-1)
    if counts is not None and c.size and (c.min() < 1 or c.max() > t_count):
        raise ValueError(f"counts must lie in 1..{t_count}")
    c = np.unique(np.concatenate([c[(c >= 1) & (c <= t_count)], [t_count]]))
    return c.astype(np.int32)


def _mean0(v: np.ndarray) -> float:
    return float(np.mean(v)) if v.size else 0.0


# ===================== Golden float64 NumPy implementation =====================
def golden_convergence(predictions, y, counts, orders) -> Dict[str, np.ndarray]:
    """For every order r and count k, the metrics of the subset ``p[orders[r, :k]]`` averaged over the
    windows, as a dict of (R, K) float64 arrays.  A window with a non-finite probability in any of its T
    passes is left out of every sum and every denominator."""
    p = M.as_2d(np.asarray(predictions)).astype(np.float64)
    yy = np.asarray(y).reshape(-1) != 0
    orders = np.asarray(orders)
    counts = np.asarray(counts).reshape(-1)
    ok = np.all(np.isfinite(p), axis=0)
    p, yy = p[:, ok], yy[ok]
    h = np.stack([M.binary_entropy_nats(pt) for pt in p])
    mean_all = np.mean(p, axis=0)
    lab_all = mean_all > 0.5
    out = {k: np.zeros((len(orders), len(counts))) for k in METRICS}
    for r, order in enumerate(orders):
        for j, k in enumerate(counts):
            sub = p[order[:k]]
            mean, var = np.mean(sub, axis=0), np.var(sub, axis=0)
            total = M.binary_entropy_nats(mean)
            expected = np.mean(h[order[:k]], axis=0)
            lab = mean > 0.5
            w = {"pred_variance": var, "total_pred_entropy": total, "expected_aleatoric_entropy": expected,
                 "mutual_info": np.maximum(total - expected, 0)}
            for key, v in M.aggregates(w, yy.astype(np.int64)).items() if p.shape[1] else ():
                out[key][r, j] = v
            out["accuracy"][r, j] = _mean0(lab == yy)
            out["flip_rate"][r, j] = _mean0(lab != lab_all)
            out["mean_abs_shift"][r, j] = _mean0(np.abs(mean - mean_all))
    return out


# ===================== Public API =====================
def on_device(predictions):
    """The predictions as a (T, N) tensor, on the GPU when there is one (the drivers and the CLI load NumPy
    dumps; the curves of a CUDA tensor come from the kernel)."""
    p2 = C._as_tensor_2d(predictions)
    return p2.to("cuda") if C._gpu_ok() and not p2.is_cuda else p2


def convergence_curves(predictions, y, counts: Optional[Sequence[int]] = None, n_orders: int = 100,
                       random_state: Optional[int] = 2025) -> Dict[str, np.ndarray]:
    """The nine ``METRICS`` as (n_orders + 1, K) float64 arrays (row 0: the passes as run; rows 1..: random
    orders), plus ``counts`` (K,) and ``orders`` (n_orders + 1, T).

    ``predictions`` is (T, N) or (T, N, 1), NumPy or a torch tensor.  ``counts`` defaults to 1, 2, 3, 5, 10,
    15, 20, 30, 40, 50, ... clipped to T; T is always appended when absent.  CUDA predictions go through
    the HIP kernel, anything else through the eager emulation of ``ops/converge.py``."""
    torch = _torch()
    from ..ops import converge as V

    p2 = C._as_tensor_2d(predictions)
    yy = C._labels(y)
    t_count, n = p2.shape
    if len(yy) != n:
        raise ValueError(f"Mismatch between prediction samples ({n}) and label samples ({len(yy)})")
    if t_count > V.MAX_T:
        raise ValueError(f"at most {V.MAX_T} passes or members, got {t_count}")
    cs = default_counts(t_count, counts)
    orders = subset_orders(t_count, n_orders, random_state)
    dev = p2.device
    args = (p2.contiguous(), torch.as_tensor(yy, device=dev), torch.as_tensor(orders, device=dev), cs.tolist())
    s = V.sums(*args) if p2.is_cuda else V.sums_eager(*args)
    out = V.finalize(s)
    out["counts"], out["orders"] = cs, orders
    return out


def _needed(counts: np.ndarray, ok: np.ndarray) -> int:
    """Smallest count from which on every count qualifies; the last count, k = T, always does."""
    ok = ok.copy()
    ok[-1] = True
    bad = np.flatnonzero(~ok)
    return int(counts[bad[-1] + 1] if bad.size else counts[0])


def evaluate_convergence(predictions, y, evaluation_label: str = "Convergence", counts: Optional[Sequence[int]] = None,
                         n_orders: int = 100, random_state: Optional[int] = 2025, tolerance: float = 0.05,
                         flip_tolerance: float = 0.01, output_dir: Optional[str] = "./uq_plots/convergence",
                         make_plots: bool = True) -> Dict[str, float]:
    """Convergence of every metric of ``METRICS`` with the count of passes / members, as one flat dictionary.

    Per metric m and count k: ``{m}_at_{k}``, the value of the order as run, and ``{m}_at_{k}_mean``,
    ``_ci_lower``, ``_ci_upper``, the mean and the 2.5 / 97.5 percentiles over the random orders.
    ``passes_needed_{m}`` is the smallest count k such that at every count k' >= k at least 95 % of the
    random orders have ``|m[r, k'] - m_T| <= tolerance |m_T|``, with m_T the all-T value; for ``flip_rate``
    the smallest k from which on the 97.5th percentile is at most ``flip_tolerance``.  k = T always
    qualifies.  With ``output_dir`` the table goes to ``convergence_{label}.csv`` and, unless ``make_plots``
    is off, one figure of the variance and entropy curves with their bands and one of the flip rate."""
    cur = convergence_curves(predictions, y, counts, n_orders, random_state)
    cs = cur["counts"]
    final: Dict[str, float] = {}
    rows = [{"N": int(k)} for k in cs]
    bands = {}
    for m in METRICS:
        v = cur[m]
        rnd = v[1:] if v.shape[0] > 1 else v
        # a mean of equal values may round one ulp away from them: keep it inside the values' range
        mean = np.clip(rnd.mean(0), rnd.min(0), rnd.max(0))
        lo, hi = np.percentile(rnd, 2.5, axis=0), np.percentile(rnd, 97.5, axis=0)
        bands[m] = (v[0], mean, lo, hi)
        for j, k in enumerate(cs):
            final[f"{m}_at_{k}"] = float(v[0, j])
            final[f"{m}_at_{k}_mean"], final[f"{m}_at_{k}_ci_lower"], final[f"{m}_at_{k}_ci_upper"] = (
                float(mean[j]), float(lo[j]), float(hi[j]))
            rows[j].update({m: float(v[0, j]), f"{m}_mean": float(mean[j]), f"{m}_lower": float(lo[j]),
                            f"{m}_upper": float(hi[j])})
        if m == "flip_rate":
            ok = hi <= flip_tolerance
        else:
            m_all = v[0, -1]
            ok = np.mean(np.abs(rnd - m_all) <= tolerance * abs(m_all), axis=0) >= 0.95
        final[f"passes_needed_{m}"] = _needed(cs, ok)
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        pd.DataFrame(rows).to_csv(os.path.join(output_dir, f"convergence_{evaluation_label}.csv"), index=False)
        if make_plots:
            plot_convergence(cs, bands, evaluation_label, output_dir)
            plot_flip_rate(cs, bands["flip_rate"], final["passes_needed_flip_rate"], evaluation_label, output_dir)
    return final


# ===================== Plots =====================
def plot_convergence(counts, bands: Dict, label: str, output_dir: str):
    """Variance and entropy curves against the count: the order as run, the mean over random orders, 95 % band."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig, axes = plt.subplots(1, 2, figsize=(12, 4.5))
    groups = (("overall_mean_variance", "mean_variance_class_0", "mean_variance_class_1"),
              ("mean_total_pred_entropy", "mean_expected_aleatoric_entropy", "mean_mutual_info"))
    for ax, keys, name in zip(axes, groups, ("Mean predictive variance", "Mean entropy (nats)")):
        for key in keys:
            run, mean, lo, hi = bands[key]
            line, = ax.plot(counts, mean, "-", label=key)
            ax.fill_between(counts, lo, hi, alpha=0.2, color=line.get_color())
            ax.plot(counts, run, "o", ms=3, color=line.get_color())
        ax.set_xlabel("Passes / members used")
        ax.set_ylabel(name)
        ax.grid(True, alpha=0.3)
        ax.legend(fontsize=8)
    fig.suptitle(f"Convergence (dots: order as run; line and band: random subsets) - {label}")
    fig.tight_layout()
    fig.savefig(os.path.join(output_dir, f"convergence_{label}.png"), bbox_inches="tight")
    plt.close(fig)


def plot_flip_rate(counts, band, needed: int, label: str, output_dir: str):
    """Share of windows whose label at k differs from the label of all T passes."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    run, mean, lo, hi = band
    fig = plt.figure(figsize=(7, 4.5))
    plt.fill_between(counts, lo, hi, alpha=0.25, label="95% of random subsets")
    plt.plot(counts, mean, "-", label="mean over random subsets")
    plt.plot(counts, run, "o", ms=3, label="order as run")
    plt.axvline(needed, color="k", linestyle="--", alpha=0.5, label=f"passes needed: {needed}")
    plt.xlabel("Passes / members used")
    plt.ylabel("Label flip rate against all passes")
    plt.title(f"Label stability - {label}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"flip_rate_{label}.png"), bbox_inches="tight")
    plt.close(fig)
