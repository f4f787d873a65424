"""Calibration and selective-prediction analysis with bootstrap confidence intervals.

Two questions the aggregate UQ metrics of ``uq_techniques.py`` leave open:

* are the probabilities calibrated?  -> :func:`calibration_metrics` (ECE, MCE, Brier score, NLL and
  the reliability-diagram bins);
* what is gained by referring the most uncertain windows to a human scorer?  ->
  :func:`selective_prediction` (accuracy / sensitivity / specificity of the retained windows as a
  function of coverage, and the area under the risk-coverage curve);

and :func:`evaluate_calibration` gives both with percentile bootstrap CIs.  Every per-window quantity
involved is invariant under resampling, so a bootstrap replicate is a gather plus a histogram of integer
records (``ops/calib.py``, ``csrc/uq_calib.hip``): one launch for all B replicates on the GPU.  The
point estimates run through the same code with one "replicate" whose indices are ``arange(n)``.

The ``golden_*`` functions are straightforward float64 NumPy implementations (no quantisation, every
replicate recomputed from the resampled arrays): the test oracle and the timing baseline.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Optional, Sequence, Union

import numpy as np

from . import metrics as M

try:  # plotting is optional (headless Agg backend)
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
except Exception:  # pragma: no cover
    plt = None

SCORES = ("pred_variance", "total_pred_entropy", "expected_aleatoric_entropy", "mutual_info")
CI_SCALARS = ("ece", "mce", "brier", "nll", "aurc")
CI_CURVES = ("accuracy", "sensitivity", "specificity")
DEFAULT_COVERAGES = np.linspace(0.5, 1.0, 11)


def _torch():
    import torch

    return torch


def _gpu_ok() -> bool:
    from .uq_techniques import _gpu_ok as ok

    return ok()


# ===================== Golden float64 NumPy implementations =====================
def golden_calibration(p, y, n_bins: int = 15) -> Dict[str, np.ndarray]:
    """ECE / MCE / Brier / NLL and the reliability bins of per-window probabilities ``p`` (float64)."""
    p = np.asarray(p, dtype=np.float64)
    y = (np.asarray(y) != 0).astype(np.float64)
    n = len(p)
    b = np.minimum(np.floor(p * n_bins).astype(np.int64), n_bins - 1)
    count = np.bincount(b, minlength=n_bins)
    conf = np.full(n_bins, np.nan)
    freq = np.full(n_bins, np.nan)
    ece, gaps = 0.0, []
    for k in range(n_bins):
        if count[k] == 0:
            continue
        conf[k] = np.mean(p[b == k])
        freq[k] = np.mean(y[b == k])
        gaps.append(abs(freq[k] - conf[k]))
        ece += count[k] / n * gaps[-1]
    pt = np.clip(p, 1e-7, 1 - 1e-7)
    return {"ece": float(ece), "mce": float(max(gaps)) if gaps else float("nan"),
            "brier": float(np.mean((p - y) ** 2)),
            "nll": float(np.mean(-(y * np.log(pt) + (1 - y) * np.log(1 - pt)))),
            "bin_count": count, "bin_confidence": conf, "bin_frequency": freq}


def _ratio(num: float, den: float) -> float:
    return num / den if den > 0 else float("nan")


def golden_selective(p, score, y, thresholds) -> Dict[str, np.ndarray]:
    """Coverage / accuracy / sensitivity / specificity of the windows with ``score <= threshold``."""
    p = np.asarray(p)
    score = np.asarray(score)
    y = (np.asarray(y) != 0).astype(np.int64)
    pred = (p > 0.5).astype(np.int64)
    cov, acc, sens, spec = [], [], [], []
    for t in thresholds:
        keep = score <= t
        yk, pk = y[keep], pred[keep]
        cov.append(keep.sum() / len(p))
        acc.append(_ratio(float(np.sum(yk == pk)), float(keep.sum())))
        sens.append(_ratio(float(np.sum((yk == 1) & (pk == 1))), float(np.sum(yk == 1))))
        spec.append(_ratio(float(np.sum((yk == 0) & (pk == 0))), float(np.sum(yk == 0))))
    out = {"coverage": np.array(cov, dtype=np.float64), "accuracy": np.array(acc, dtype=np.float64),
           "sensitivity": np.array(sens, dtype=np.float64), "specificity": np.array(spec, dtype=np.float64)}
    ok = ~(np.isnan(out["coverage"]) | np.isnan(out["accuracy"]))
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    out["aurc"] = float(trapezoid(1.0 - out["accuracy"][ok], out["coverage"][ok])) if ok.any() else float("nan")
    return out


def golden_replicates(p, score, y, thresholds, idx, n_bins: int = 15) -> Dict[str, np.ndarray]:
    """Every metric recomputed from the resampled arrays for each row of ``idx`` (B, n)."""
    p, score, y = np.asarray(p), np.asarray(score), np.asarray(y)
    rows = []
    for ix in idx:
        r = golden_calibration(p[ix], y[ix], n_bins)
        r.update(golden_selective(p[ix], score[ix], y[ix], thresholds))
        rows.append(r)
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]} if rows else {}


# ===================== Per-window inputs =====================
def _as_tensor_2d(predictions):
    torch = _torch()
    p = predictions if isinstance(predictions, torch.Tensor) else torch.as_tensor(np.asarray(predictions))
    if p.dim() == 3 and p.shape[-1] == 1:
        p = p[..., 0]
    if p.dim() == 1:
        p = p.reshape(1, -1)
    if p.dim() != 2:
        raise ValueError("predictions must be (T, N), (T, N, 1) or (N,)")
    return p.float()


def per_window(predictions, score: Union[str, np.ndarray] = "total_pred_entropy", device: Optional[str] = None):
    """(mean probability, score) as fp32 tensors on ``device``, from ``ops.uq.metrics``."""
    torch = _torch()
    from ..ops import uq as uq_ops

    p2 = _as_tensor_2d(predictions)
    if device is not None:
        p2 = p2.to(device)
    m = uq_ops.metrics(p2.contiguous())
    if isinstance(score, str):
        if score not in SCORES:
            raise ValueError(f"score must be one of {SCORES} or an (N,) array")
        s = m[uq_ops.ROW_NAMES.index(score)]
    else:
        s = torch.as_tensor(np.asarray(score.cpu() if isinstance(score, torch.Tensor) else score)).float().reshape(-1)
        if s.numel() != m.shape[1]:
            raise ValueError("score must have one value per window")
        s = s.to(m.device)
    return m[uq_ops.MEAN].contiguous(), s.contiguous()


def coverage_thresholds(score, coverages) -> np.ndarray:
    """Threshold j = the ceil(c_j n)-th smallest score: an order statistic, no interpolation."""
    torch = _torch()
    s = score if isinstance(score, torch.Tensor) else torch.as_tensor(np.asarray(score))
    n = s.numel()
    c = np.sort(np.asarray(coverages, dtype=np.float64).reshape(-1))
    if c.size and (c[0] <= 0 or c[-1] > 1):
        raise ValueError("coverages must lie in (0, 1]")
    k = np.clip(np.ceil(c * n - 1e-9).astype(np.int64), 1, n)
    srt = torch.sort(s.float()).values
    return srt[torch.as_tensor(k - 1, device=srt.device)].cpu().numpy().astype(np.float32)


def _labels(y_true) -> np.ndarray:
    torch = _torch()
    y = np.asarray(y_true.cpu() if isinstance(y_true, torch.Tensor) else y_true).reshape(-1)
    return (y != 0).astype(np.int32)


def _use_device(predictions) -> bool:
    torch = _torch()
    return (isinstance(predictions, torch.Tensor) and predictions.is_cuda) or _gpu_ok()


def _records(p, s, y, thr, n_bins):
    """Per-window records: the HIP kernel when ``p`` is on the GPU, else the eager emulation."""
    torch = _torch()
    from ..ops import calib

    return calib.prep(p, s, torch.as_tensor(y, device=p.device), torch.as_tensor(thr, device=p.device), n_bins)


def _point(rec, n_bins, n_thr) -> Dict[str, np.ndarray]:
    """Point estimates: one "replicate" that draws every window once."""
    torch = _torch()
    from ..ops import calib

    n = rec.shape[0]
    idx = torch.arange(n, dtype=torch.int32, device=rec.device)[None]
    return calib.finalize(calib.bootstrap_sums(rec, 1, n_bins, n_thr, idx=idx)[0], n, n_bins, n_thr)


# ===================== Public API =====================
def calibration_metrics(predictions, y, n_bins: int = 15) -> Dict:
    """``ece``, ``mce``, ``brier``, ``nll`` and the arrays ``bin_count``, ``bin_confidence``,
    ``bin_frequency`` of the mean prediction."""
    dev = "cuda" if _use_device(predictions) else None
    p, s = per_window(predictions, "pred_variance", dev)
    r = _point(_records(p, s, _labels(y), np.zeros(0, np.float32), n_bins), n_bins, 0)
    out = {k: float(r[k]) for k in ("ece", "mce", "brier", "nll")}
    out.update({k: r[k] for k in ("bin_count", "bin_confidence", "bin_frequency")})
    return out


def selective_prediction(predictions, y, score: Union[str, np.ndarray] = "total_pred_entropy",
                         coverages: Sequence[float] = DEFAULT_COVERAGES) -> Dict:
    """Retain the windows whose uncertainty is at most the threshold of each nominal coverage; returns
    ``thresholds``, the ``coverage`` actually achieved (ties can exceed the nominal value),
    ``accuracy``, ``sensitivity``, ``specificity`` and ``aurc``."""
    dev = "cuda" if _use_device(predictions) else None
    p, s = per_window(predictions, score, dev)
    thr = coverage_thresholds(s, coverages)
    r = _point(_records(p, s, _labels(y), thr, 1), 1, len(thr))
    return {"thresholds": thr, "coverage": r["coverage"], "accuracy": r["accuracy"], "sensitivity": r["sensitivity"],
            "specificity": r["specificity"], "aurc": float(r["aurc"])}


def coverage_suffixes(coverages) -> list:
    """Key suffixes such as ``_at_0.80``, with as many decimals as keep them distinct."""
    c = np.sort(np.asarray(coverages, dtype=np.float64).reshape(-1))
    for nd in (2, 3, 4, 6):
        out = [f"_at_{v:.{nd}f}" for v in c]
        if len(set(out)) == len(out):
            break
    return out


def _ci(vals: np.ndarray, alpha: float = 0.05):
    """Mean and percentile interval over the non-NaN replicates (all NaN -> NaN)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return (float(np.nanmean(vals)), float(np.nanpercentile(vals, 100 * alpha / 2)),
                float(np.nanpercentile(vals, 100 * (1 - alpha / 2))))


def evaluate_calibration(predictions, y, evaluation_label: str = "Calibration", n_bootstrap: int = 100,
                         random_state: Optional[int] = None, parity: bool = True,
                         score: Union[str, np.ndarray] = "total_pred_entropy", n_bins: int = 15,
                         coverages: Sequence[float] = DEFAULT_COVERAGES, output_plot_dir: str = "./uq_plots",
                         make_plots: bool = True) -> Dict[str, float]:
    """Calibration + selective prediction with bootstrap CIs, as one flat dictionary.

    Point values ``ece``, ``mce``, ``brier``, ``nll``, ``aurc`` and, per nominal coverage,
    ``coverage_at_X``, ``accuracy_at_X``, ``sensitivity_at_X``, ``specificity_at_X``; for every one of
    these but the coverage also ``{m}_mean``, ``{m}_ci_lower``, ``{m}_ci_upper`` (the convention of
    ``metrics.confidence_intervals``, NaN replicates ignored).  ``parity=True`` resamples with
    ``metrics.parity_bootstrap_indices``, ``parity=False`` with the device counter hash, i.e. the same
    resamples as ``bootstrap_metrics`` for the same ``random_state``.
    """
    from ..ops import calib

    dev = "cuda" if _use_device(predictions) else None
    p, s = per_window(predictions, score, dev)
    yy = _labels(y)
    n = p.numel()
    if len(yy) != n:
        raise ValueError(f"Mismatch between prediction samples ({n}) and label samples ({len(yy)})")
    thr = coverage_thresholds(s, coverages)
    rec = _records(p, s, yy, thr, n_bins)
    pt = _point(rec, n_bins, len(thr))
    idx = None
    if parity:
        idx = _torch().as_tensor(M.parity_bootstrap_indices(n, n_bootstrap, random_state).astype(np.int32),
                                 device=rec.device)
    sums = calib.bootstrap_sums(rec, n_bootstrap, n_bins, len(thr), idx=idx,
                                seed=0 if random_state is None else random_state)
    boot = calib.finalize(sums, n, n_bins, len(thr))
    suf = coverage_suffixes(coverages)
    final: Dict[str, float] = {}
    for k in CI_SCALARS:
        final[k] = float(pt[k])
        if n_bootstrap:
            final[f"{k}_mean"], final[f"{k}_ci_lower"], final[f"{k}_ci_upper"] = _ci(boot[k])
    for j, sfx in enumerate(suf):
        final[f"coverage{sfx}"] = float(pt["coverage"][j])
        for k in CI_CURVES:
            final[f"{k}{sfx}"] = float(pt[k][j])
            if n_bootstrap:
                (final[f"{k}{sfx}_mean"], final[f"{k}{sfx}_ci_lower"],
                 final[f"{k}{sfx}_ci_upper"]) = _ci(boot[k][:, j])
    if make_plots:
        plot_reliability(pt, boot if n_bootstrap else None, evaluation_label, output_plot_dir)
        plot_accuracy_coverage(pt, boot if n_bootstrap else None, evaluation_label, output_plot_dir)
    return final


# ===================== Plots =====================
def _band(vals: np.ndarray, alpha: float = 0.05):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.nanpercentile(vals, 100 * alpha / 2, axis=0), np.nanpercentile(vals, 100 * (1 - alpha / 2), axis=0)


def plot_reliability(pt: Dict, boot: Optional[Dict], uq_name: str, output_dir: str = "./uq_plots"):
    """Reliability diagram: observed frequency against mean confidence per bin, with the CI band."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    ok = pt["bin_count"] > 0
    fig = plt.figure(figsize=(6, 6))
    plt.plot([0, 1], [0, 1], "k--", alpha=0.5, label="Perfect calibration")
    if boot is not None:
        lo, hi = _band(boot["bin_frequency"])
        plt.fill_between(pt["bin_confidence"][ok], lo[ok], hi[ok], alpha=0.25, label="95% CI")
    plt.plot(pt["bin_confidence"][ok], pt["bin_frequency"][ok], "o-", label=f"ECE {float(pt['ece']):.4f}")
    plt.xlabel("Mean predicted probability")
    plt.ylabel("Observed frequency of apnea/hypopnea")
    plt.title(f"Reliability diagram - {uq_name}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"reliability_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)


def plot_accuracy_coverage(pt: Dict, boot: Optional[Dict], uq_name: str, output_dir: str = "./uq_plots"):
    """Accuracy of the retained windows against coverage, with the CI band."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(7, 5))
    if boot is not None:
        lo, hi = _band(boot["accuracy"])
        plt.fill_between(pt["coverage"], lo, hi, alpha=0.25, label="95% CI")
    plt.plot(pt["coverage"], pt["accuracy"], "o-", label=f"AURC {float(pt['aurc']):.4f}")
    plt.xlabel("Coverage (fraction of windows retained)")
    plt.ylabel("Accuracy of retained windows")
    plt.title(f"Accuracy vs coverage - {uq_name}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"accuracy_coverage_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)
