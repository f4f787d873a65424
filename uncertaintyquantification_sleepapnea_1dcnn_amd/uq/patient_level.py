"""Patient-level apnea severity with uncertainty, and the patient-cluster bootstrap.

The clinical endpoint of sleep-apnea screening is per patient: events per hour of the whole night,
read off at 5 / 15 / 30 per hour.  With T stochastic passes for every window the posterior of a
patient's index is at hand: :func:`patient_table` gives its mean, a credible interval, the
severity-class probabilities and whether the severity is ambiguous; :func:`cohort_metrics` scores a
cohort (Bland-Altman agreement, severity accuracy and weighted kappa, interval coverage, ...).

Windows of one patient are strongly correlated, so a bootstrap that resamples windows
(``uq_techniques.bootstrap_metrics``, ``calibration.evaluate_calibration``) gives intervals that are too
narrow.  :func:`cluster_bootstrap_metrics` and :func:`evaluate_patient_level` resample patients.  Both rest
on one segmented reduction of the (T, N) predictions by patient (``ops/patient.py``,
``csrc/uq_patient.hip``): per-patient integer sums, after which a replicate costs P additions instead of
N gathers and all B replicates are one launch.

The ``golden_*`` functions are plain float64 NumPy from the raw probabilities (no quantisation, no
integer tables; every replicate recomputed from the gathered windows): the test oracle and the timing
baseline.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

from . import calibration as C
from . import metrics as M

plt = C.plt

SEVERITY = ("normal", "mild", "moderate", "severe")
DEFAULT_CUTOFFS = (5.0, 15.0, 30.0)
COHORT_KEYS = ("index_mae", "index_bias", "index_loa_lower", "index_loa_upper", "severity_accuracy",
               "severity_within_one", "severity_kappa_linear", "ci_coverage", "share_confident",
               "severity_accuracy_confident", "pearson_r_accuracy_entropy", "accuracy", "sensitivity",
               "specificity") + M.AGG_KEYS


def _torch():
    import torch

    return torch


def _ids(patient_ids) -> np.ndarray:
    torch = _torch()
    ids = np.asarray(patient_ids.cpu() if isinstance(patient_ids, torch.Tensor) else patient_ids).reshape(-1)
    return ids


def _severity(index: np.ndarray, cutoffs: Sequence[float]) -> np.ndarray:
    """Class 0..3: the number of cutoffs that the index reaches (5 <= mild < 15 <= moderate < 30 <= severe)."""
    c = np.asarray(cutoffs, dtype=np.float64)
    if c.shape != (3,) or not np.all(np.diff(c) > 0):
        raise ValueError("cutoffs must be three increasing values")
    return np.sum(np.asarray(index, dtype=np.float64)[..., None] >= c, axis=-1).astype(np.int64)


# ===================== Golden float64 NumPy implementations =====================
def golden_patient_table(predictions, y_true, patient_ids, window_seconds: float = 60.0,
                         cutoffs: Sequence[float] = DEFAULT_CUTOFFS, ci: float = 0.95,
                         min_agreement: float = 0.9) -> pd.DataFrame:
    """The table of :func:`patient_table`, patient by patient from the raw probabilities in float64."""
    p = M.as_2d(np.asarray(predictions)).astype(np.float64)
    y = (np.asarray(y_true).reshape(-1) != 0).astype(np.int64)
    ids = _ids(patient_ids)
    w = M.per_window(p)
    bits = M.binary_entropy_bits(w["mean_pred"])
    label = (w["mean_pred"] > 0.5).astype(np.int64)
    alpha = 1.0 - ci
    rows = []
    for pid in np.unique(ids):
        k = np.flatnonzero(ids == pid)
        n = len(k)
        per_pass = np.array([np.sum(pt[k] > 0.5) / n * 3600 / window_seconds for pt in p])
        true_index = np.sum(y[k]) / n * 3600 / window_seconds
        pred_index = np.sum(label[k]) / n * 3600 / window_seconds
        cls = _severity(per_pass, cutoffs)
        share = np.array([np.mean(cls == c) for c in range(4)])
        nz = share[share > 0]
        yk, lk = y[k], label[k]
        rows.append({
            "Patient_ID": pid, "num_windows": n, "num_passes": p.shape[0], "hours": n * window_seconds / 3600,
            "true_index": true_index, "true_severity": int(_severity(true_index, cutoffs)),
            "pred_index": pred_index, "pred_severity": int(_severity(pred_index, cutoffs)),
            "index_mean": float(np.mean(per_pass)), "index_std": float(np.std(per_pass)),
            "index_ci_lower": float(np.percentile(per_pass, 100 * alpha / 2)),
            "index_ci_upper": float(np.percentile(per_pass, 100 * (1 - alpha / 2))),
            "p_normal": share[0], "p_mild": share[1], "p_moderate": share[2], "p_severe": share[3],
            "severity_entropy": float(-np.sum(nz * np.log(nz))),
            "severity_confident": bool(share.max() >= min_agreement),
            "patient_accuracy": float(np.mean(yk == lk)),
            "sensitivity": float(np.mean(lk[yk == 1] == 1)) if np.any(yk == 1) else 0.0,
            "specificity": float(np.mean(lk[yk == 0] == 0)) if np.any(yk == 0) else 0.0,
            "mean_variance": float(np.mean(w["pred_variance"][k])),
            "mean_entropy": float(np.mean(bits[k])),
        })
    return pd.DataFrame(rows)


def golden_cohort(table: pd.DataFrame, predictions, y_true, patient_ids, draws=None) -> Dict[str, float]:
    """Cohort metrics of the patients ``draws`` (positions in ``table``, repeats allowed; default: every
    patient once): the per-patient part from the table rows, the pooled part from the drawn patients'
    windows, concatenated."""
    p = M.as_2d(np.asarray(predictions))
    y = (np.asarray(y_true).reshape(-1) != 0).astype(np.int64)
    ids = _ids(patient_ids)
    uniq = np.unique(ids)
    draws = np.arange(len(uniq)) if draws is None else np.asarray(draws)
    t = table.iloc[draws]
    e = (t["pred_index"] - t["true_index"]).to_numpy(np.float64)
    n_pat = len(e)
    sd = float(np.std(e, ddof=1)) if n_pat > 1 else 0.0
    tc, pc = t["true_severity"].to_numpy(np.int64), t["pred_severity"].to_numpy(np.int64)
    conf = np.zeros((4, 4))
    for a, b in zip(tc, pc):
        conf[a, b] += 1
    wgt = np.array([[1.0 - abs(i - j) / 3.0 for j in range(4)] for i in range(4)])
    po = float(np.sum(wgt * conf) / n_pat)
    pe = float(np.sum(wgt * np.outer(conf.sum(1), conf.sum(0))) / n_pat ** 2)
    sure = t["severity_confident"].to_numpy(bool)
    inside = ((t["index_ci_lower"] <= t["true_index"]) & (t["true_index"] <= t["index_ci_upper"])).to_numpy(bool)
    acc, ent = t["patient_accuracy"].to_numpy(np.float64), t["mean_entropy"].to_numpy(np.float64)
    out = {
        "index_mae": float(np.mean(np.abs(e))), "index_bias": float(np.mean(e)),
        "index_loa_lower": float(np.mean(e) - 1.96 * sd), "index_loa_upper": float(np.mean(e) + 1.96 * sd),
        "severity_accuracy": float(np.mean(tc == pc)), "severity_within_one": float(np.mean(np.abs(tc - pc) <= 1)),
        "severity_kappa_linear": (po - pe) / (1.0 - pe) if pe < 1.0 else 0.0,
        "ci_coverage": float(np.mean(inside)), "share_confident": float(np.mean(sure)),
        "severity_accuracy_confident": float(np.mean(tc[sure] == pc[sure])) if sure.any() else float("nan"),
        "pearson_r_accuracy_entropy": (float(np.corrcoef(acc, ent)[0, 1])
                                       if n_pat > 1 and np.ptp(acc) > 0 and np.ptp(ent) > 0 else float("nan")),
    }
    win = {pid: np.flatnonzero(ids == pid) for pid in uniq[np.unique(draws)]}
    ix = np.concatenate([win[uniq[d]] for d in draws])
    w = M.per_window(p[:, ix])
    yy, lab = y[ix], (w["mean_pred"] > 0.5).astype(np.int64)
    out["accuracy"] = float(np.mean(yy == lab))
    out["sensitivity"] = float(np.mean(lab[yy == 1] == 1)) if np.any(yy == 1) else 0.0
    out["specificity"] = float(np.mean(lab[yy == 0] == 0)) if np.any(yy == 0) else 0.0
    out.update(M.aggregates(w, yy))
    return out


def golden_cluster_replicates(table: pd.DataFrame, predictions, y_true, patient_ids, idx) -> List[Dict[str, float]]:
    """:func:`golden_cohort` of every row of ``idx`` (B, P): the drawn patients' windows are gathered and
    everything is computed again."""
    return [golden_cohort(table, predictions, y_true, patient_ids, draws=row) for row in np.asarray(idx)]


# ===================== Integer path =====================
class PatientRecord:
    """The (P, 25) int64 per-patient record of a table, boxed: ``DataFrame.attrs`` are compared and printed
    by pandas, which a bare array does not survive."""

    def __init__(self, array: np.ndarray):
        self.array = array

    def __len__(self) -> int:
        return len(self.array)

    def __repr__(self) -> str:
        return f"PatientRecord({self.array.shape[0]} patients)"


def _tables(predictions, y_true, patient_ids):
    """Patient ids (sorted unique), ``pass_pos`` (T, P) and ``rec`` (P, 12) as int64 NumPy, device used."""
    torch = _torch()
    from ..ops import patient as P
    from ..ops import uq as uq_ops

    p2 = C._as_tensor_2d(predictions)
    y = C._labels(y_true)
    ids = _ids(patient_ids)
    n = p2.shape[1]
    if len(y) != n or len(ids) != n:
        raise ValueError(f"Mismatch between prediction samples ({n}), labels ({len(y)}) and patient ids ({len(ids)})")
    if n == 0:
        raise ValueError("no windows")
    uniq, inv = np.unique(ids, return_inverse=True)
    if C._use_device(predictions):
        p2 = p2.to("cuda")
    p2 = p2.contiguous()
    m = uq_ops.metrics(p2)
    dev = p2.device
    pass_pos, rec = P.reduce(p2, m, torch.as_tensor(y, device=dev),
                             torch.as_tensor(inv.reshape(-1).astype(np.int32), device=dev), len(uniq))
    return uniq, pass_pos.cpu().numpy().astype(np.int64), rec.cpu().numpy().astype(np.int64), dev


def _patient_record(rec: np.ndarray, table: pd.DataFrame) -> np.ndarray:
    """(P, 25) int64 per-patient record of ``ops/patient.py``: ``rec`` plus the derived integers, built in
    float64 from the integer counts."""
    from ..ops import patient as P

    n, n1, pp = (rec[:, i].astype(np.float64) for i in (0, 1, 2))
    err = (pp - n1) / n
    tc, pc = table["true_severity"].to_numpy(np.int64), table["pred_severity"].to_numpy(np.int64)
    inside = ((table["index_ci_lower"] <= table["true_index"]) & (table["true_index"] <= table["index_ci_upper"]))
    sure = table["severity_confident"].to_numpy(bool)
    err_q = np.rint(err * P.Q_SCALE).astype(np.int64)
    a = np.rint(table["patient_accuracy"].to_numpy(np.float64) * P.MOM_SCALE).astype(np.int64)
    e = np.rint(table["mean_entropy"].to_numpy(np.float64) * P.MOM_SCALE).astype(np.int64)
    extra = np.stack([tc, pc, err_q, np.abs(err_q), np.rint(err * err * P.Q_SCALE).astype(np.int64),
                      inside.to_numpy(bool).astype(np.int64), sure.astype(np.int64),
                      (sure & (tc == pc)).astype(np.int64), a, e, a * a, e * e, a * e], axis=1)
    return np.concatenate([rec, extra], axis=1).astype(np.int64)


def _table_from(uniq, pass_pos, rec, window_seconds, cutoffs, ci, min_agreement) -> pd.DataFrame:
    from ..ops import patient as P

    if not window_seconds > 0:
        raise ValueError("window_seconds must be positive")
    if not 0 < ci < 1:
        raise ValueError("ci must lie in (0, 1)")
    c = {k: rec[:, i].astype(np.float64) for i, k in enumerate(P.REC_COLS)}
    n = c["n"]
    if np.any(n <= 0):
        raise ValueError("a patient without windows")
    # (P, T), passes along the contiguous axis: NumPy then sums a patient's passes as it sums a 1-D array
    per_pass = np.ascontiguousarray(pass_pos.T).astype(np.float64) / n[:, None] * 3600 / window_seconds
    true_index = c["n_y1"] / n * 3600 / window_seconds
    pred_index = c["pred_pos"] / n * 3600 / window_seconds
    cls = _severity(per_pass, cutoffs)
    share = np.stack([np.mean(cls == k, axis=1) for k in range(4)], axis=1)     # (P, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        sev_ent = -np.sum(np.where(share > 0, share * np.log(np.where(share > 0, share, 1.0)), 0.0), axis=1)
    alpha = 1.0 - ci
    n0 = n - c["n_y1"]
    table = pd.DataFrame({
        "Patient_ID": uniq, "num_windows": rec[:, 0], "num_passes": pass_pos.shape[0],
        "hours": n * window_seconds / 3600,
        "true_index": true_index, "true_severity": _severity(true_index, cutoffs),
        "pred_index": pred_index, "pred_severity": _severity(pred_index, cutoffs),
        "index_mean": np.mean(per_pass, axis=1), "index_std": np.std(per_pass, axis=1),
        "index_ci_lower": np.percentile(per_pass, 100 * alpha / 2, axis=1),
        "index_ci_upper": np.percentile(per_pass, 100 * (1 - alpha / 2), axis=1),
        "p_normal": share[:, 0], "p_mild": share[:, 1], "p_moderate": share[:, 2], "p_severe": share[:, 3],
        "severity_entropy": sev_ent + 0.0,
        "severity_confident": share.max(axis=1) >= min_agreement,
        "patient_accuracy": c["correct"] / n,
        "sensitivity": P._div0(c["tp"], c["n_y1"]),
        "specificity": P._div0(c["correct"] - c["tp"], n0),
        "mean_variance": c["var_q"] / P.Q_SCALE / n,
        "mean_entropy": c["ent_bits_q"] / P.Q_SCALE / n,
    })
    table.attrs["patient_record"] = PatientRecord(_patient_record(rec, table))
    table.attrs["window_seconds"] = float(window_seconds)
    return table


# ===================== Public API =====================
def patient_table(predictions, y_true, patient_ids, window_seconds: float = 60.0,
                  cutoffs: Sequence[float] = DEFAULT_CUTOFFS, ci: float = 0.95,
                  min_agreement: float = 0.9) -> pd.DataFrame:
    """One row per patient: the window apnea index with its posterior over the T passes.

    The *window apnea index* is positive windows per hour of recording, ``count / n * 3600 /
    window_seconds``: each positive window counts as one event.  The reference labels a window positive
    on at least 10 s of apnea / hypopnea overlap, so this is a proxy of the apnea-hypopnea index, capped
    at 60 per hour for 60 s windows.  The predicted and the true index follow the same rule and compare
    like with like.  It is meaningful on the unbalanced test set only, not after SMOTE / RUS.

    Columns: ``Patient_ID, num_windows, num_passes, hours, true_index, true_severity`` (0 normal, 1 mild,
    2 moderate, 3 severe at ``cutoffs``); ``pred_index, pred_severity`` from the mean prediction, as
    ``Predicted_Label``; ``index_mean, index_std, index_ci_lower, index_ci_upper`` over the T per-pass
    indices (``ci`` percentile interval; with ``num_passes`` = 1 the interval is a point);
    ``p_normal .. p_severe``, the share of passes in each class, their ``severity_entropy`` (nats) and
    ``severity_confident`` (modal share >= ``min_agreement``); ``patient_accuracy, sensitivity,
    specificity`` (0.0 on a zero denominator); ``mean_variance, mean_entropy`` (bits) as in
    ``analysis.patient.aggregate_patient_uq_metrics``.  Patients are ordered by ``np.unique`` of the ids.
    The integer record behind the table travels in ``table.attrs`` for :func:`cohort_metrics`."""
    uniq, pass_pos, rec, _ = _tables(predictions, y_true, patient_ids)
    return _table_from(uniq, pass_pos, rec, window_seconds, cutoffs, ci, min_agreement)


def _sums(prec: np.ndarray, n_boot: int, idx, seed: int, device):
    torch = _torch()
    from ..ops import patient as P

    pt = torch.as_tensor(prec, device=device)
    it = None if idx is None else torch.as_tensor(np.asarray(idx).astype(np.int32), device=device)
    return P.bootstrap_sums(pt, n_boot, idx=it, seed=seed)


def _point_sums(prec: np.ndarray, device):
    """Point estimate: one "replicate" that draws every patient once."""
    return _sums(prec, 1, np.arange(prec.shape[0])[None], 0, device)[0]


def cohort_metrics(table_or_sums, window_seconds: Optional[float] = None) -> Dict[str, float]:
    """Cohort metrics of a :func:`patient_table` (or of one (41,) vector of ``ops.patient`` sums):
    ``index_mae, index_bias, index_loa_lower, index_loa_upper`` (Bland-Altman, bias -+ 1.96 sd);
    ``severity_accuracy, severity_within_one, severity_kappa_linear``; ``ci_coverage``;
    ``share_confident, severity_accuracy_confident``; ``pearson_r_accuracy_entropy``; pooled ``accuracy,
    sensitivity, specificity`` and the six ``metrics.AGG_KEYS`` over all windows."""
    from ..ops import patient as P

    if isinstance(table_or_sums, pd.DataFrame):
        prec = table_or_sums.attrs.get("patient_record")
        if prec is None or len(prec) != len(table_or_sums):
            raise ValueError("cohort_metrics needs a table made by patient_table (its integer record is in attrs)")
        window_seconds = table_or_sums.attrs["window_seconds"] if window_seconds is None else window_seconds
        sums = _point_sums(prec.array, "cuda" if C._gpu_ok() else "cpu")
    else:
        sums = table_or_sums
        if getattr(sums, "ndim", 1) != 1:
            raise ValueError("cohort_metrics takes one (41,) vector of sums; use ops.patient.finalize for replicates")
    r = P.finalize(sums, 3600.0 / (60.0 if window_seconds is None else window_seconds))
    return {k: float(r[k]) for k in COHORT_KEYS}


def _draws(n_pat: int, n_bootstrap: int, random_state: Optional[int], parity: bool):
    return M.parity_bootstrap_indices(n_pat, n_bootstrap, random_state) if parity else None


def cluster_bootstrap_metrics(predictions, y_true, patient_ids, n_bootstrap: int = 100,
                              random_state: Optional[int] = None, parity: bool = True) -> List[Dict[str, float]]:
    """B patient-cluster bootstrap replicates of the six ``metrics.AGG_KEYS``: the result has the shape of
    ``uq_techniques.bootstrap_metrics`` and goes to ``compute_confidence_intervals`` likewise, but a
    replicate draws P patients with replacement and takes all their windows.  ``parity=True`` draws with
    ``metrics.parity_bootstrap_indices(P, B, seed)``, else the device counter hash."""
    from ..ops import patient as P

    uniq, pass_pos, rec, dev = _tables(predictions, y_true, patient_ids)
    table = _table_from(uniq, pass_pos, rec, 60.0, DEFAULT_CUTOFFS, 0.95, 0.9)
    sums = _sums(table.attrs["patient_record"].array, n_bootstrap, _draws(len(uniq), n_bootstrap, random_state, parity),
                 0 if random_state is None else random_state, dev)
    r = P.finalize(sums, 60.0)
    return [{k: float(r[k][b]) for k in M.AGG_KEYS} for b in range(n_bootstrap)]


def evaluate_patient_level(predictions, y_true, patient_ids, evaluation_label: str = "Patient level",
                           n_bootstrap: int = 100, random_state: Optional[int] = 2025, parity: bool = True,
                           output_dir: Optional[str] = None, make_plots: bool = True,
                           window_seconds: float = 60.0, cutoffs: Sequence[float] = DEFAULT_CUTOFFS,
                           ci: float = 0.95, min_agreement: float = 0.9) -> Dict[str, float]:
    """Cohort metrics with patient-cluster bootstrap intervals, as one flat dictionary: every key of
    :func:`cohort_metrics` plus ``{m}_ci_lower`` / ``{m}_ci_upper`` (percentiles over the non-NaN
    replicates).  With ``output_dir`` the table goes to ``patient_severity_{label}.csv`` and, unless
    ``make_plots`` is off, a Bland-Altman plot and the severity confusion matrix next to it."""
    from ..ops import patient as P

    uniq, pass_pos, rec, dev = _tables(predictions, y_true, patient_ids)
    table = _table_from(uniq, pass_pos, rec, window_seconds, cutoffs, ci, min_agreement)
    prec = table.attrs["patient_record"].array
    per_hour = 3600.0 / window_seconds
    pt = P.finalize(_point_sums(prec, dev), per_hour)
    final: Dict[str, float] = {k: float(pt[k]) for k in COHORT_KEYS}
    if n_bootstrap:
        sums = _sums(prec, n_bootstrap, _draws(len(uniq), n_bootstrap, random_state, parity),
                     0 if random_state is None else random_state, dev)
        boot = P.finalize(sums, per_hour)
        for k in COHORT_KEYS:
            _, final[f"{k}_ci_lower"], final[f"{k}_ci_upper"] = C._ci(boot[k])
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        table.to_csv(os.path.join(output_dir, f"patient_severity_{evaluation_label}.csv"), index=False)
        if make_plots:
            plot_bland_altman(table, final, evaluation_label, output_dir)
            plot_severity_confusion(pt["confusion"], evaluation_label, output_dir)
    return final


# ===================== Plots =====================
def plot_bland_altman(table: pd.DataFrame, metrics: Dict[str, float], label: str, output_dir: str):
    """Predicted - true index against their mean, with the bias and the limits of agreement."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(7, 5))
    plt.scatter((table["pred_index"] + table["true_index"]) / 2, table["pred_index"] - table["true_index"], s=14, alpha=0.7)
    for key, style in (("index_bias", "k-"), ("index_loa_lower", "r--"), ("index_loa_upper", "r--")):
        plt.axhline(metrics[key], color=style[0], linestyle=style[1:], label=f"{key} {metrics[key]:.2f}")
    plt.xlabel("Mean of predicted and true window apnea index (events / h)")
    plt.ylabel("Predicted - true (events / h)")
    plt.title(f"Bland-Altman - {label}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"bland_altman_{label}.png"), bbox_inches="tight")
    plt.close(fig)


def plot_severity_confusion(confusion: np.ndarray, label: str, output_dir: str):
    """4 x 4 counts of true (rows) against predicted (columns) severity."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(5.5, 5))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plt.imshow(confusion, cmap="Blues")
    for i in range(4):
        for j in range(4):
            plt.text(j, i, str(int(confusion[i, j])), ha="center", va="center")
    plt.xticks(range(4), SEVERITY)
    plt.yticks(range(4), SEVERITY)
    plt.xlabel("Predicted severity")
    plt.ylabel("True severity")
    plt.title(f"Severity confusion - {label}")
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"severity_confusion_{label}.png"), bbox_inches="tight")
    plt.close(fig)
