"""Discrimination: ROC / PR AUC and the Mann-Whitney U with bootstrap confidence intervals.

Two rank questions of the thesis, each so far answered by one point value on the host:

* does the classifier separate apnea from normal windows?  ``task="apnea"`` ranks the mean probability
  against the label (``roc_auc`` / ``auc_pr`` of ``evaluation.classification_metrics``);
* does uncertainty separate wrong predictions from right ones?  ``task="error"`` ranks an uncertainty
  score against "prediction wrong" (the U statistic of ``analysis.stats.entropy_mannwhitney``).

:func:`evaluate_discrimination` gives both with percentile bootstrap intervals, over windows or, with
``patient_ids``, over patients (the cluster bootstrap of ``uq.patient_level``: windows of one patient are
correlated and window intervals come out several times too narrow).  :func:`compare_discrimination`
evaluates two prediction sets on the same resamples and reports paired differences.

Resampling does not change the order of the scores: the windows are sorted once and every replicate is a
row of integer weights over the sorted windows, scanned on the GPU (``ops/rank.py``, ``csrc/uq_rank.hip``).
The point estimates run through the same code with the weight row of ones.

The ``golden_*`` functions are the float64 oracle: scikit-learn and SciPy on the literal resample.

Multi-rank: rank statistics are not additive over window shards.  Under a multi-rank group the drivers
gather the per-window predictions (the API gather path of the other analyses) and these functions compute
from the gathered values on the calling rank; a distributed scan is out of scope.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple, Union

import numpy as np

from . import calibration as C
from . import metrics as M

plt = C.plt

TASKS = ("apnea", "error")
METRICS = ("auroc", "pr_auc", "average_precision", "u_statistic")


def _torch():
    import torch

    return torch


# ===================== Golden float64 oracle (scikit-learn / SciPy) =====================
def golden_discrimination(score, target) -> Dict[str, float]:
    """``auroc``, ``pr_auc`` (trapezoid of ``precision_recall_curve``), ``average_precision``, the
    Mann-Whitney ``u_statistic`` of positives against negatives with its one-sided asymptotic ``p_value``
    (positives greater), ``n_pos`` and ``n_neg``, of the windows with a finite score.  With one class
    absent the ratios and the p-value are NaN and U is 0."""
    from scipy.stats import mannwhitneyu
    from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_auc_score

    s = np.asarray(score, dtype=np.float64).reshape(-1)
    t = np.asarray(target).reshape(-1) != 0
    ok = np.isfinite(s)
    s, t = s[ok], t[ok]
    n_pos, n_neg = int(t.sum()), int((~t).sum())
    out = {"auroc": float("nan"), "pr_auc": float("nan"), "average_precision": float("nan"), "u_statistic": 0.0,
           "p_value": float("nan"), "n_pos": n_pos, "n_neg": n_neg}
    if n_pos == 0 or n_neg == 0:
        return out
    prec, rec, _ = precision_recall_curve(t, s)
    u, p = mannwhitneyu(s[t], s[~t], alternative="greater", method="asymptotic")
    out.update(auroc=float(roc_auc_score(t, s)), pr_auc=float(auc(rec, prec)),
               average_precision=float(average_precision_score(t, s)), u_statistic=float(u), p_value=float(p))
    return out


def golden_replicates(score, target, idx) -> Dict[str, np.ndarray]:
    """:func:`golden_discrimination` of the literal resample ``score[ix], target[ix]`` for every row of ``idx``."""
    s, t = np.asarray(score).reshape(-1), np.asarray(target).reshape(-1)
    rows = [golden_discrimination(s[ix], t[ix]) for ix in np.asarray(idx)]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]} if rows else {}


# ===================== Scores and targets =====================
def task_inputs(predictions, y, task: str = "apnea", score: Union[str, np.ndarray] = "total_pred_entropy",
                device: Optional[str] = None):
    """(score, target) tensors of a task: the mean probability against the label (``apnea``) or the
    uncertainty ``score`` (a ``per_window`` row name or an (N,) array) against "prediction wrong" (``error``)."""
    torch = _torch()
    if task not in TASKS:
        raise ValueError(f"task must be one of {TASKS}")
    by_name = isinstance(score, str)
    p, s = C.per_window(predictions, score if task == "error" and by_name else "pred_variance", device)
    yy = torch.as_tensor(C._labels(y), device=p.device)
    if yy.numel() != p.numel():
        raise ValueError(f"Mismatch between prediction samples ({p.numel()}) and label samples ({yy.numel()})")
    if task == "error" and not by_name:  # an array keeps its precision: float64 scores rank as float64
        a = np.asarray(score.cpu() if isinstance(score, torch.Tensor) else score).reshape(-1)
        if a.size != p.numel():
            raise ValueError("score must have one value per window")
        s = torch.as_tensor(a.astype(np.float64 if a.dtype == np.float64 else np.float32), device=p.device)
    if task == "apnea":
        return p, yy
    return s, ((p > 0.5).to(yy.dtype) != yy).to(torch.int32)


def _device(predictions) -> Optional[str]:
    return "cuda" if C._use_device(predictions) else None


def _point_sums(pr):
    torch = _torch()
    from ..ops import rank

    n = pr["n_valid"]
    buf = torch.ones(1, (n + 3) // 4 * 4, dtype=torch.int32, device=pr["packed"].device)
    return rank.scan_sums(buf[:, :n], pr["packed"])[0]


def p_value_greater(u2: int, n_pos: int, n_neg: int, group_sizes: np.ndarray) -> float:
    """One-sided p-value (positives greater) of ``U = u2 / 2``: SciPy's asymptotic method, the normal
    approximation with tie and continuity correction.  The tie term comes from the tie-group sizes, on the host."""
    from scipy.stats import norm

    if n_pos == 0 or n_neg == 0:
        return float("nan")
    n = n_pos + n_neg
    t = np.asarray(group_sizes, dtype=np.float64)
    tie_term = float(np.sum(t ** 3 - t))
    mu = n_pos * n_neg / 2
    s = np.sqrt(n_pos * n_neg / 12 * ((n + 1) - tie_term / (n * (n - 1))))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.float64(u2 / 2 - mu - 0.5) / s
    return float(norm.sf(z))


def _group_sizes(pr) -> np.ndarray:
    torch = _torch()
    from ..ops import rank

    starts = torch.nonzero((pr["packed"] & rank.START_BIT) != 0).reshape(-1).cpu().numpy()
    return np.diff(np.append(starts, pr["n_valid"]))


class _Draws:
    """The resamples of one call, shared by every task and prediction set evaluated in it."""

    def __init__(self, n: int, n_bootstrap: int, random_state: Optional[int], parity: bool, patient_ids, device):
        torch = _torch()
        from ..ops import rank
        from ..ops.calib import _hash_row

        self.n_boot, self.seed = int(n_bootstrap), 0 if random_state is None else int(random_state)
        self.idx = self.mult = self.code = None
        if patient_ids is None:
            if parity and n_bootstrap:
                self.idx = torch.as_tensor(M.parity_bootstrap_indices(n, n_bootstrap, random_state).astype(np.int32),
                                           device=device)
            return
        ids = np.asarray(patient_ids.cpu() if isinstance(patient_ids, torch.Tensor) else patient_ids).reshape(-1)
        if len(ids) != n:
            raise ValueError(f"Mismatch between prediction samples ({n}) and patient ids ({len(ids)})")
        uniq, inv, counts = np.unique(ids, return_inverse=True, return_counts=True)
        n_pat = len(uniq)
        rank.check_cluster_limit(n_pat, int(counts.max()) if n_pat else 0)
        if parity:
            draws = torch.as_tensor(M.parity_bootstrap_indices(n_pat, n_bootstrap, random_state).astype(np.int64))
        else:  # the counter hash of patient_bootstrap_kernel with n = P
            seed = self.seed & 0xFFFFFFFF
            draws = torch.stack([_hash_row(n_pat, b, seed, "cpu") for b in range(n_bootstrap)]) if n_bootstrap else \
                torch.zeros(0, n_pat, dtype=torch.int64)
        self.mult = rank.multiplicities(draws.reshape(n_bootstrap, -1), n_pat).to(device)
        self.code = torch.as_tensor(inv.reshape(-1).astype(np.int64), device=device)

    def sums(self, pr, splits: int = 0):
        from ..ops import rank

        return rank.bootstrap_sums(pr, self.n_boot, idx=self.idx, seed=self.seed, splits=splits, mult=self.mult,
                                   code=self.code)


def _evaluate_task(predictions, y, task, score, draws: Optional[_Draws], device) -> Tuple[Dict, Dict, Dict]:
    """(point metrics, replicate arrays, prep) of one task."""
    from ..ops import rank

    s, t = task_inputs(predictions, y, task, score, device)
    pr = rank.prep(s, t)
    sums = _point_sums(pr) if pr["n_valid"] else np.zeros(len(rank.COLS), np.int64)
    pt = rank.finalize(sums)
    point = {k: float(pt[k]) for k in METRICS}
    point.update(n_pos=int(pt["n_pos"]), n_neg=int(pt["n_neg"]), n_valid=pr["n_valid"],
                 p_value=p_value_greater(int(sums[rank.U2_COL]), int(pt["n_pos"]), int(pt["n_neg"]), _group_sizes(pr)))
    boot = rank.finalize(draws.sums(pr)) if draws is not None and draws.n_boot else {}
    return point, boot, pr


# ===================== Public API =====================
def discrimination_metrics(predictions, y, task: str = "apnea",
                           score: Union[str, np.ndarray] = "total_pred_entropy") -> Dict[str, float]:
    """Point estimates of one task: ``auroc``, ``pr_auc``, ``average_precision``, ``u_statistic`` (the
    Mann-Whitney U of the positives' scores against the negatives'), its one-sided ``p_value`` (positives
    greater; asymptotic, with tie and continuity correction), ``n_pos``, ``n_neg`` and ``n_valid`` (windows
    with a finite score; the others are dropped)."""
    return _evaluate_task(predictions, y, task, score, None, _device(predictions))[0]


def discrimination_replicates(predictions, y, task: str = "apnea", score: Union[str, np.ndarray] = "total_pred_entropy",
                              n_bootstrap: int = 100, random_state: Optional[int] = 2025, parity: bool = True,
                              patient_ids=None) -> Dict[str, np.ndarray]:
    """(B,) float64 arrays of ``METRICS`` (and ``n_pos``, ``n_neg``, ``groups``) over the bootstrap replicates."""
    dev = _device(predictions)
    n = C._as_tensor_2d(predictions).shape[1]
    draws = _Draws(n, n_bootstrap, random_state, parity, patient_ids, dev or "cpu")
    return _evaluate_task(predictions, y, task, score, draws, dev)[1]


def evaluate_discrimination(predictions, y, evaluation_label: str = "Discrimination", n_bootstrap: int = 100,
                            random_state: Optional[int] = 2025, parity: bool = True, patient_ids=None,
                            score: Union[str, np.ndarray] = "total_pred_entropy",
                            output_plot_dir: str = "./uq_plots", make_plots: bool = True) -> Dict[str, float]:
    """Both tasks with bootstrap CIs, as one flat dictionary.

    Per task (prefix ``apnea_`` / ``error_``) and metric m of ``METRICS``: ``{m}``, ``{m}_mean``,
    ``{m}_ci_lower``, ``{m}_ci_upper`` (the convention of ``metrics.confidence_intervals``; replicates
    without positives or without negatives are NaN and ignored), plus ``p_value``, ``n_pos``, ``n_neg``
    and ``n_valid``.  ``parity=True`` resamples with ``metrics.parity_bootstrap_indices``, ``parity=False``
    with the device counter hash (the resamples of ``bootstrap_metrics`` for the same ``random_state``).
    ``patient_ids`` switches to the patient-cluster bootstrap, with the draws of
    ``patient_level.cluster_bootstrap_metrics`` for the same seed.  Unless ``make_plots`` is off, the ROC and
    the PR curve of either task are drawn from the host golden, with the interval in the legend."""
    dev = _device(predictions)
    n = C._as_tensor_2d(predictions).shape[1]
    draws = _Draws(n, n_bootstrap, random_state, parity, patient_ids, dev or "cpu")
    final: Dict[str, float] = {}
    for task in TASKS:
        point, boot, _ = _evaluate_task(predictions, y, task, score, draws, dev)
        for k, v in point.items():
            final[f"{task}_{k}"] = v
        if n_bootstrap:
            for k in METRICS:
                (final[f"{task}_{k}_mean"], final[f"{task}_{k}_ci_lower"],
                 final[f"{task}_{k}_ci_upper"]) = C._ci(boot[k])
        if make_plots:
            s, t = task_inputs(predictions, y, task, score, dev)
            plot_curves(s.cpu().numpy(), t.cpu().numpy(), final, task, evaluation_label, output_plot_dir)
    return final


def compare_discrimination(predictions_a, predictions_b, y, n_bootstrap: int = 100, random_state: Optional[int] = 2025,
                           parity: bool = True, patient_ids=None,
                           score: Union[str, np.ndarray] = "total_pred_entropy",
                           score_b: Union[None, str, np.ndarray] = None, return_replicates: bool = False):
    """Paired comparison of two prediction sets over the same windows, on the same resamples.

    Per task and metric m: ``{task}_{m}_a``, ``{task}_{m}_b``, the difference ``{task}_{m}_diff`` (a - b)
    with ``_diff_mean``, ``_diff_ci_lower``, ``_diff_ci_upper`` (percentiles of the replicate-wise
    differences) and ``{task}_{m}_share_a_gt_b``, the share of the replicates (valid for both) with a > b.
    ``score_b`` is the uncertainty score of the second set (default: as ``score``).  With
    ``return_replicates`` the replicate-wise differences come back as a second dictionary."""
    dev = "cuda" if (C._use_device(predictions_a) or C._use_device(predictions_b)) else None
    n = C._as_tensor_2d(predictions_a).shape[1]
    if C._as_tensor_2d(predictions_b).shape[1] != n:
        raise ValueError("the two prediction sets must cover the same windows")
    draws = _Draws(n, n_bootstrap, random_state, parity, patient_ids, dev or "cpu")
    final: Dict[str, float] = {}
    reps: Dict[str, np.ndarray] = {}
    for task in TASKS:
        pa, ba, _ = _evaluate_task(predictions_a, y, task, score, draws, dev)
        pb, bb, _ = _evaluate_task(predictions_b, y, task, score if score_b is None else score_b, draws, dev)
        for k in METRICS:
            key = f"{task}_{k}"
            final[f"{key}_a"], final[f"{key}_b"], final[f"{key}_diff"] = pa[k], pb[k], pa[k] - pb[k]
            if n_bootstrap:
                d = ba[k] - bb[k]
                reps[key] = d
                final[f"{key}_diff_mean"], final[f"{key}_diff_ci_lower"], final[f"{key}_diff_ci_upper"] = C._ci(d)
                ok = ~np.isnan(d)
                final[f"{key}_share_a_gt_b"] = float(np.mean(d[ok] > 0)) if ok.any() else float("nan")
    return (final, reps) if return_replicates else final


# ===================== Plots =====================
def plot_curves(score, target, final: Dict[str, float], task: str, uq_name: str, output_dir: str = "./uq_plots"):
    """Point ROC and PR curves of one task (scikit-learn on the host), the bootstrap interval in the legend."""
    if plt is None:
        return
    from sklearn.metrics import precision_recall_curve, roc_curve

    s = np.asarray(score, dtype=np.float64)
    t = np.asarray(target) != 0
    ok = np.isfinite(s)
    s, t = s[ok], t[ok]
    if t.sum() == 0 or (~t).sum() == 0:
        return
    os.makedirs(output_dir, exist_ok=True)

    def legend(k, name):
        v = final[f"{task}_{k}"]
        lo, hi = final.get(f"{task}_{k}_ci_lower"), final.get(f"{task}_{k}_ci_upper")
        return f"{name} {v:.4f}" + (f" [{lo:.4f}, {hi:.4f}]" if lo is not None else "")

    what = "apnea vs normal" if task == "apnea" else "wrong vs right predictions"
    fpr, tpr, _ = roc_curve(t, s)
    fig = plt.figure(figsize=(6, 6))
    plt.plot([0, 1], [0, 1], "k--", alpha=0.5)
    plt.plot(fpr, tpr, label=legend("auroc", "AUROC"))
    plt.xlabel("False positive rate")
    plt.ylabel("True positive rate")
    plt.title(f"ROC ({what}) - {uq_name}")
    plt.legend(loc="lower right")
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"roc_{task}_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)
    prec, rec, _ = precision_recall_curve(t, s)
    fig = plt.figure(figsize=(6, 6))
    plt.plot(rec, prec, label=legend("pr_auc", "PR AUC"))
    plt.xlabel("Recall")
    plt.ylabel("Precision")
    plt.title(f"Precision-recall ({what}) - {uq_name}")
    plt.legend(loc="lower left")
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"pr_{task}_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)
