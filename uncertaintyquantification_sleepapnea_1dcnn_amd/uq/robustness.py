"""Uncertainty under signal corruption: degraded copies of the test windows and one table over (corruption, severity).

Every other analysis assumes test windows that look like the training windows.  This one asks the question of
Ovadia et al. (2019, "Can you trust your model's uncertainty?") of the three samplers: what do accuracy, calibration,
uncertainty and conformal coverage do when the SpO2 probe slips, a belt saturates, a channel goes flat or the
channels lose sync?

* :func:`corrupt_windows` degrades windows ``(N, L, C)`` with one condition; the kinds, their severity table, the
  sigma-relative units and the counter-hash randomness are defined in ``ops/shift.py`` (HIP kernel
  ``csrc/uq_shift.hip`` on the GPU, its float64 emulation elsewhere).  The result is re-standardised per window
  like the pipeline (``restandardize=True``), deterministic in ``(seed, kind, channel, global window index)`` and
  independent of sharding (``window_offset``).  All severities of a kind share their draws, so curves over severity
  are paired.
* :func:`shift_conditions` lists (kind, severity) conditions; :func:`evaluate_shift` predicts every condition with
  ``predict_fn(X) -> (T, N, 1)`` (:func:`mc_dropout_predictor`, :func:`deep_ensemble_predictor`,
  :func:`laplace_predictor` wrap the samplers) and returns one row per condition plus the clean row (severity 0,
  re-standardisation only); :func:`plot_shift` draws one figure per kind, one curve per method.

Under ``bn_mode="batch"`` (the reference's ``model(x, training=True)``) the BatchNorm statistics of a condition are
those of the *corrupted* set: that is the reference's semantics and part of the finding, not an artefact of the sweep.
Under ``torchrun`` nothing new is needed: the samplers shard the windows themselves and the keys hold global indices.

Not built: corruption of raw signals before resampling, physiological artefact models, a fused corrupt-and-infer path.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from . import calibration as C
from . import metrics as M

plt = C.plt

KINDS = ("gaussian_noise", "flatline", "spikes", "drift", "clip", "delay", "quantize")
CONFORMAL_COLUMNS = ("coverage", "coverage_class_0", "coverage_class_1", "share_empty", "share_both")
CALIBRATION_COLUMNS = ("ece", "mce", "brier", "nll")
PLOT_COLUMNS = (("accuracy", "Accuracy"), ("ece", "ECE"), ("mean_total_pred_entropy", "Mean predictive entropy (nats)"),
                ("detection_auroc", "Detection AUROC (corrupted vs clean)"))
LAUNCH_BYTES = 1 << 30     # output bytes of one corruption launch of evaluate_shift (K conditions at a time)


class ShiftCondition(NamedTuple):
    """One condition: ``p`` is the kind's parameter (from the severity table, or given), ``channels`` None = all."""
    kind: str
    severity: Optional[int]
    p: float
    channels: Optional[Tuple[int, ...]]


CLEAN = ShiftCondition("none", 0, 0.0, None)


def _torch():
    import torch

    return torch


def _ops():
    from ..ops import shift

    return shift


# ===================== Corruption =====================
def make_condition(kind: str, severity: Optional[int] = None, p: Optional[float] = None,
                   channels: Optional[Sequence[int]] = None) -> ShiftCondition:
    ops = _ops()
    code, pv, _ = ops.condition(kind, severity, p, None)
    ch = None if channels is None else tuple(int(c) for c in channels)
    return ShiftCondition(ops.KINDS[code], None if severity is None else int(severity), pv, ch)


def shift_conditions(kinds: Sequence[str] = KINDS, severities: Sequence[int] = (1, 2, 3, 4, 5),
                     channels: Optional[Sequence[int]] = None) -> List[ShiftCondition]:
    """Every (kind, severity) pair, kinds outermost; ``channels`` restricts all of them (None: every channel)."""
    return [make_condition(k, severity=s, channels=channels) for k in kinds for s in severities]


def _condition_arrays(conds: Sequence[ShiftCondition], n_channels: int):
    ops = _ops()
    kinds = [ops.kind_code(c.kind) for c in conds]
    params = [float(c.p) for c in conds]
    masks = [ops.channel_mask(c.channels, n_channels) for c in conds]
    return kinds, params, masks


def _use_gpu(x) -> bool:
    torch = _torch()
    return (isinstance(x, torch.Tensor) and x.is_cuda) or (not isinstance(x, torch.Tensor) and C._gpu_ok())


def corrupt_conditions(X, conds: Sequence[ShiftCondition], seed: int = 2025, window_offset: int = 0,
                       restandardize: bool = True):
    """(K, N, L, C) fp32 of the same type and device as ``X``: every condition of every window.  A NumPy array is
    corrupted on the GPU when there is one."""
    torch = _torch()
    ops = _ops()
    is_t = isinstance(X, torch.Tensor)
    x = X if is_t else torch.as_tensor(np.ascontiguousarray(X))
    if x.dtype not in (torch.float32, torch.float64):
        x = x.float()
    if x.dim() != 3:
        raise ValueError("X must be (N, L, C)")
    if not is_t and _use_gpu(X):
        x = x.cuda()
    out = ops.shift_corrupt(x, *_condition_arrays(conds, x.shape[2]), int(seed), int(window_offset), restandardize)
    return out if is_t else out.cpu().numpy()


def corrupt_windows(X, kind: str, severity: Optional[int] = None, p: Optional[float] = None,
                    channels: Optional[Sequence[int]] = None, seed: int = 2025, window_offset: int = 0,
                    restandardize: bool = True):
    """Windows ``(N, L, C)`` degraded by one condition, fp32, same type and device as ``X``.

    ``severity`` 1..5 picks the parameter from the table of ``ops/shift.py`` (0: re-standardisation only); a float
    ``p`` may be given instead.  ``channels`` restricts the kind to some channels (default all, independent draws per
    channel).  ``window_offset`` is the global index of ``X[0]``: a shard's result is the slice of the whole set's."""
    return corrupt_conditions(X, [make_condition(kind, severity, p, channels)], seed, window_offset, restandardize)[0]


# ===================== Predictors =====================
def mc_dropout_predictor(model, n_pred: int = 50, bn_mode: str = "batch", seed: Optional[int] = 2025,
                         as_numpy: bool = True) -> Callable:
    """``predict_fn`` of MC Dropout.  Every call starts from the pass counter the model had when the predictor was
    made, so every condition sees the same dropout masks (with ``seed``) and the curves over severity are paired."""
    from . import uq_techniques as U

    base = model._call_counter

    def predict(X):
        model._call_counter = base
        return U.mc_dropout_predict(model, X, n_pred=n_pred, bn_mode=bn_mode, seed=seed, as_numpy=as_numpy)

    return predict


def deep_ensemble_predictor(models: List, as_numpy: bool = True) -> Callable:
    from . import uq_techniques as U

    return lambda X: U.deep_ensembles_predict(models, X, as_numpy=as_numpy)


def laplace_predictor(model, state, n_samples: int = 50, seed: int = 2025, as_numpy: bool = True) -> Callable:
    from .laplace import laplace_predict

    return lambda X: laplace_predict(model, state, X, n_samples=n_samples, seed=seed, as_numpy=as_numpy)


# ===================== Evaluation =====================
def _detection_auroc(score_corrupted, score_clean) -> float:
    """AUROC of the score on the corrupted copies (positives) against the clean copies of the same windows."""
    torch = _torch()
    s = torch.cat([score_corrupted, score_clean])
    t = torch.cat([torch.ones_like(score_corrupted, dtype=torch.int32), torch.zeros_like(score_clean, dtype=torch.int32)])
    if s.is_cuda:
        from ..ops import rank
        from .discrimination import _point_sums

        pr = rank.prep(s, t)
        return float(rank.finalize(_point_sums(pr))["auroc"]) if pr["n_valid"] else float("nan")
    from .discrimination import golden_discrimination

    return golden_discrimination(s.numpy(), t.numpy())["auroc"]


def _channels_label(channels) -> str:
    return "all" if channels is None else ",".join(str(c) for c in channels)


def _row(cond: ShiftCondition, preds, y, score, clean, conformal, n_bootstrap, seed, codes) -> Tuple[Dict, Dict]:
    from . import uq_techniques as U

    dev = "cuda" if C._use_device(preds) else None
    p, s = C.per_window(preds, score, dev)
    pn = p.double().cpu().numpy()
    pred = pn > 0.5
    pos, neg = y == 1, y == 0
    row = {"kind": cond.kind, "severity": cond.severity, "p": cond.p, "channels": _channels_label(cond.channels),
           "accuracy": float(np.mean(pred == pos)),
           "sensitivity": float(np.mean(pred[pos])) if pos.any() else float("nan"),
           "specificity": float(np.mean(~pred[neg])) if neg.any() else float("nan")}
    cal = C.calibration_metrics(preds, y)
    row.update({k: cal[k] for k in CALIBRATION_COLUMNS})
    w = U.uq_evaluation_dist(preds, y)
    row.update(M.aggregates(w, y))
    if clean is None:
        clean = {"p": pn, "score": s}
    row["flip_rate_vs_clean"] = float(np.mean(pred != (clean["p"] > 0.5)))
    row["mean_abs_shift_vs_clean"] = float(np.mean(np.abs(pn - clean["p"])))
    row["detection_auroc"] = _detection_auroc(s, clean["score"])
    if codes is not None:
        hit, tot = np.bincount(codes, weights=(pred == pos)), np.bincount(codes)
        row["patient_macro_accuracy"] = float(np.mean(hit[tot > 0] / tot[tot > 0]))
    if conformal is not None:
        from .conformal import conformal_metrics

        cm = conformal_metrics(conformal.predict_sets(preds), y, valid=np.isfinite(pn))
        row.update({k: cm[k] for k in CONFORMAL_COLUMNS})
    if n_bootstrap:
        boot = C.evaluate_calibration(preds, y, n_bootstrap=n_bootstrap, random_state=seed, score=score, make_plots=False)
        for k in CALIBRATION_COLUMNS:
            row[f"{k}_ci_lower"], row[f"{k}_ci_upper"] = boot[f"{k}_ci_lower"], boot[f"{k}_ci_upper"]
    return row, clean


def evaluate_shift(predict_fn: Callable, X, y, conditions: Optional[Sequence[ShiftCondition]] = None, seed: int = 2025,
                   patient_ids=None, score: Union[str, np.ndarray] = "total_pred_entropy", conformal=None,
                   n_bootstrap: int = 0, output_dir: Optional[str] = None, label: str = "shift") -> pd.DataFrame:
    """One row per condition plus the clean row (first; severity 0 = re-standardisation only).

    Columns: ``kind``, ``severity``, ``p``, ``channels``; ``accuracy``, ``sensitivity``, ``specificity`` of the mean
    probability at 0.5; ``ece``, ``mce``, ``brier``, ``nll`` (:func:`calibration_metrics`); the six aggregates of
    ``uq_evaluation_dist``; ``flip_rate_vs_clean`` and ``mean_abs_shift_vs_clean`` against the clean row's mean
    probability; ``detection_auroc``, the AUROC of ``score`` on the corrupted copies against the clean copies of the
    same windows (0.5 in the clean row); with ``patient_ids`` ``patient_macro_accuracy``; with ``conformal`` (a
    ``ConformalPredictor`` calibrated on clean data) ``coverage``, ``coverage_class_0/1``, ``share_empty``,
    ``share_both``; with ``n_bootstrap > 0`` the ``_ci_lower`` / ``_ci_upper`` of the calibration metrics from the
    bootstrap of :func:`evaluate_calibration`.  ``output_dir``: ``{label}.csv`` and one figure per kind."""
    torch = _torch()
    conds = list(shift_conditions() if conditions is None else conditions)
    yy = C._labels(y)
    n = len(X)
    if len(yy) != n:
        raise ValueError(f"Mismatch between windows ({n}) and label samples ({len(yy)})")
    codes = None
    if patient_ids is not None:
        ids = np.asarray(patient_ids.cpu() if isinstance(patient_ids, torch.Tensor) else patient_ids).reshape(-1)
        if len(ids) != n:
            raise ValueError(f"Mismatch between windows ({n}) and patient ids ({len(ids)})")
        codes = np.unique(ids, return_inverse=True)[1].reshape(-1)
    per = max(1, int(np.prod(np.shape(X))) * 4)
    k_launch = int(max(1, min(_ops().MAX_K, LAUNCH_BYTES // per)))
    todo = [CLEAN] + conds
    rows, clean = [], None
    for i in range(0, len(todo), k_launch):
        chunk = todo[i: i + k_launch]
        Xc = corrupt_conditions(X, chunk, seed)
        for cond, xk in zip(chunk, Xc):
            row, clean = _row(cond, predict_fn(xk), yy, score, clean, conformal, n_bootstrap, seed, codes)
            rows.append(row)
        del Xc
    table = pd.DataFrame(rows)
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        table.to_csv(os.path.join(output_dir, f"{label}.csv"), index=False)
        plot_shift({label: table}, output_dir)
    return table


# ===================== Plots =====================
def plot_shift(tables, output_dir: str = "./uq_plots") -> List[str]:
    """One figure per kind: accuracy, ECE, mean entropy and detection AUROC against severity (0 = clean), one curve
    per entry of ``tables`` (a DataFrame, or ``{method: DataFrame}``).  Rows given by ``p`` without a severity are
    left out.  Returns the paths written."""
    if plt is None:
        return []
    if isinstance(tables, pd.DataFrame):
        tables = {"": tables}
    os.makedirs(output_dir, exist_ok=True)
    kinds = []
    for t in tables.values():
        kinds += [k for k in t["kind"].unique() if k != "none" and k not in kinds]
    paths = []
    for kind in kinds:
        fig, axes = plt.subplots(1, len(PLOT_COLUMNS), figsize=(4.2 * len(PLOT_COLUMNS), 3.6))
        for name, t in tables.items():
            for ch in t.loc[t["kind"] == kind, "channels"].unique():
                sel = t[((t["kind"] == kind) & (t["channels"] == ch) | (t["kind"] == "none")) & t["severity"].notna()]
                sel = sel.sort_values("severity")
                lab = (name + (f" ch {ch}" if ch != "all" else "")).strip() or None
                for ax, (col, _) in zip(axes, PLOT_COLUMNS):
                    ax.plot(sel["severity"], sel[col], marker="o", label=lab)
        for ax, (_, title) in zip(axes, PLOT_COLUMNS):
            ax.set_xlabel("severity")
            ax.set_title(title, fontsize=9)
            ax.grid(alpha=0.3)
        if axes[0].get_legend_handles_labels()[0]:
            axes[0].legend(fontsize=8)
        fig.suptitle(f"Shift robustness: {kind}")
        fig.tight_layout()
        path = os.path.join(output_dir, f"shift_{kind}.png")
        fig.savefig(path, dpi=120)
        plt.close(fig)
        paths.append(path)
    return paths
