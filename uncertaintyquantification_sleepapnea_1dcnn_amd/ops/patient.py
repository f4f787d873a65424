"""Patient-level sums and the patient-cluster bootstrap (``csrc/uq_patient.hip``) with a bit-compatible
eager emulation.

``reduce`` turns a shard's ``(T, n)`` probabilities, its ``(7, n)`` ``ops.uq.metrics`` rows, labels and
patient codes into ``pass_pos`` (T, P) int32, the windows with ``p > 0.5`` per pass and patient, and
``rec`` (P, 12) int64 per-patient sums.  ``bootstrap_sums`` draws P patients with replacement per
replicate and returns (B, 41) int64 sums of the (P, 25) per-patient records (``rec`` plus the derived
integers that ``uq/patient_level.py`` builds on the host); ``finalize`` is the only place where these
integers become float64 metrics.  Everything in between is integer arithmetic: results do not depend on
the grid, on scheduling, on the window order or on the sharding, and shards add exactly.

``rec`` columns (fixed point: ``rint(x 2^30)``, NaN -> 0, ``|x|`` clamped to 4)::

    0 n   1 n_y1   2 pred_pos   3 tp   4 correct          counts; the prediction is the LABEL row of m
    5 VAR   6 VAR | y = 0   7 VAR | y = 1   8 ENT_NATS   9 EXP_ENT   10 MI   11 ENT_BITS

per-patient record = ``rec`` + ::

    12 true severity class   13 predicted severity class  (0..3)
    14 err   15 |err|   16 err^2      err = (pred_pos - n_y1) / n, rint(. 2^30); events per hour in finalize
    17 true index inside the credible interval   18 severity confident   19 confident and class correct
    20 a   21 e   22 a^2   23 e^2   24 a e     a = rint(accuracy 2^20), e = rint(mean entropy bits 2^20);
                                               the products are exact integers (Pearson moments)

and the sums carry the columns above followed by the 4 x 4 confusion counts at ``25 + 4 true + pred``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _ext
from . import uq as uq_ops
from .rng import boot_row

# shared with the kernels (uq_patient.hip kPatScale / kPatClamp / kPatRec / kPatFields)
Q_BITS = 30
Q_SCALE = 1 << Q_BITS
Q_CLAMP = 4.0                 # |x_q| <= 2^32, so 2^27 windows keep every sum below 2^59
MOM_BITS = 20                 # accuracy / mean-entropy quanta of the Pearson moments
MOM_SCALE = 1 << MOM_BITS
MAX_N = 1 << 27
MAX_T = 1 << 16
MAX_P_REDUCE = 1 << 24
MAX_P = 1 << 20               # bootstrap: with P max|prec| < 2^63, checked on the data

REC_COLS = ("n", "n_y1", "pred_pos", "tp", "correct", "var_q", "var0_q", "var1_q", "ent_nats_q", "exp_ent_q",
            "mi_q", "ent_bits_q")
N_REC = len(REC_COLS)
PREC_COLS = REC_COLS + ("true_class", "pred_class", "err_q", "abs_err_q", "sq_err_q", "in_ci", "confident",
                        "confident_correct", "acc_m", "ent_m", "acc2_m", "ent2_m", "accent_m")
N_PREC = len(PREC_COLS)       # 25
TRUE_CLASS, PRED_CLASS = PREC_COLS.index("true_class"), PREC_COLS.index("pred_class")
N_CLASS = 4
N_SUMS = N_PREC + N_CLASS * N_CLASS   # 41
COL = {k: i for i, k in enumerate(PREC_COLS)}


def _check_reduce(t_count: int, n: int, n_pat: int) -> None:
    if not 1 <= t_count <= MAX_T:
        raise ValueError(f"T must be in 1..{MAX_T}")
    if not 1 <= n <= MAX_N:
        raise ValueError(f"between 1 and {MAX_N} windows")
    if not (1 <= n_pat <= MAX_P_REDUCE and t_count * n_pat < (1 << 31)):
        raise ValueError(f"P must be in 1..{MAX_P_REDUCE} with T P < 2^31")


def quantise(x: torch.Tensor) -> torch.Tensor:
    """``pat_q`` of the kernel: rint(x 2^30) in float64 of the fp32 value, NaN -> 0, clamped to +-4."""
    xf = torch.nan_to_num(x.float(), nan=0.0, posinf=Q_CLAMP, neginf=-Q_CLAMP).clamp(-Q_CLAMP, Q_CLAMP)
    return torch.round(xf.double() * Q_SCALE).long()


def reduce_eager(probs: torch.Tensor, m: torch.Tensor, y: torch.Tensor, code: torch.Tensor,
                 n_pat: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The integer arithmetic of ``patient_reduce_kernel`` in torch (any device)."""
    t_count, n = probs.shape
    _check_reduce(t_count, n, n_pat)
    dev = probs.device
    c = code.long().to(dev)
    ok = (c >= 0) & (c < n_pat)
    c = c[ok]
    pos = (probs.float() > 0.5)[:, ok].to(torch.int32)
    pass_pos = torch.zeros(t_count, n_pat, dtype=torch.int32, device=dev).index_add_(1, c, pos)
    mm = m.float()[:, ok]
    yy = (y.to(dev)[ok] != 0).long()
    pred = (mm[uq_ops.LABEL] > 0.5).long()
    vq = quantise(mm[uq_ops.VAR])
    cols = [torch.ones_like(yy), yy, pred, yy * pred, (yy == pred).long(), vq, vq * (1 - yy), vq * yy,
            quantise(mm[uq_ops.ENT_NATS]), quantise(mm[uq_ops.EXP_ENT]), quantise(mm[uq_ops.MI]),
            quantise(mm[uq_ops.ENT_BITS])]
    rec = torch.zeros(n_pat, N_REC, dtype=torch.int64, device=dev).index_add_(0, c, torch.stack(cols, dim=1))
    return pass_pos, rec


def reduce(probs: torch.Tensor, m: torch.Tensor, y: torch.Tensor, code: torch.Tensor,
           n_pat: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(T, n) probabilities, (7, n) ``ops.uq.metrics`` rows, (n,) labels, (n,) patient codes in [0, P)
    -> ``pass_pos`` (T, P) int32 and ``rec`` (P, 12) int64.  The HIP kernel on the GPU.  Windows whose
    code is outside [0, P) are skipped.  The outputs of shards add to those of the whole."""
    _check_reduce(probs.shape[0], probs.shape[1], n_pat)
    if probs.is_cuda:
        dev = probs.device
        return tuple(_ext.ops().patient_reduce(probs.float().contiguous(), m.float().contiguous(), y.to(dev),
                                               code.to(dev, torch.int32).contiguous(), int(n_pat)))
    return reduce_eager(probs, m, y, code, n_pat)


def _check_prec(prec: torch.Tensor) -> None:
    if prec.dim() != 2 or prec.shape[1] != N_PREC or prec.dtype != torch.int64:
        raise ValueError(f"prec must be (P, {N_PREC}) int64")
    n_pat = prec.shape[0]
    if not 1 <= n_pat <= MAX_P:
        raise ValueError(f"P must be in 1..{MAX_P}")
    if int(prec.abs().max()) > ((1 << 63) - 1) // n_pat:
        raise ValueError("P max|prec| must stay below 2^63")


def bootstrap_sums_eager(prec: torch.Tensor, idx: Optional[torch.Tensor], seed: int, n_boot: int) -> torch.Tensor:
    """(B, 41) int64 sums of ``patient_bootstrap_kernel`` in torch."""
    _check_prec(prec)
    n_pat, dev = prec.shape[0], prec.device
    cell = (prec[:, TRUE_CLASS] & 3) * N_CLASS + (prec[:, PRED_CLASS] & 3)
    out = torch.zeros(n_boot, N_SUMS, dtype=torch.int64, device=dev)
    for b in range(n_boot):
        k = boot_row(n_pat, b, seed, dev) if idx is None else idx[b].long().to(dev)
        k = k[(k >= 0) & (k < n_pat)]
        out[b, :N_PREC] = prec[k].sum(0)
        out[b, N_PREC:] = torch.bincount(cell[k], minlength=N_CLASS * N_CLASS)
    return out


def bootstrap_sums(prec: torch.Tensor, n_boot: int, idx: Optional[torch.Tensor] = None, seed: int = 0) -> torch.Tensor:
    """(B, 41) int64 sums over P draws of patients per replicate.  ``idx`` (B, P) gives the draws, else
    the counter hash of ``ops.uq.bootstrap`` with n = P and the same ``seed``."""
    _check_prec(prec)
    seed = int(seed) & 0xFFFFFFFF
    if prec.is_cuda:
        return _ext.ops().patient_bootstrap(prec.contiguous(), None if idx is None else idx.to(prec.device), seed,
                                            int(n_boot))
    return bootstrap_sums_eager(prec, idx, seed, n_boot)


def _div0(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a / b with 0.0 where b == 0 (``metrics.class_mean``)."""
    return np.where(b > 0, a / np.where(b > 0, b, 1), 0.0)


KAPPA_W = 1.0 - np.abs(np.arange(N_CLASS)[:, None] - np.arange(N_CLASS)[None, :]) / (N_CLASS - 1.0)


def finalize(sums, per_hour: float) -> Dict[str, np.ndarray]:
    """(B, 41) or (41,) integer sums -> float64 cohort metrics (arrays with a leading B axis for 2-D input).

    ``per_hour = 3600 / window_seconds`` turns a fraction of windows into events per hour.  Bland-Altman:
    ``index_bias`` is the mean of predicted - true index, the limits are bias -+ 1.96 sd with the sample
    standard deviation (0 for fewer than two patients).  ``severity_kappa_linear`` is 0.0 when the
    expected agreement is 1, ``severity_accuracy_confident`` NaN without a confident patient, and
    ``pearson_r_accuracy_entropy`` NaN at zero variance (decided exactly, on integers)."""
    s = sums.cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    single = s.ndim == 1
    s = np.atleast_2d(s).astype(np.int64)
    if s.shape[1] != N_SUMS:
        raise ValueError(f"sums do not have {N_SUMS} columns")
    f = {k: s[:, i].astype(np.float64) for k, i in COL.items()}
    conf = s[:, N_PREC:].reshape(-1, N_CLASS, N_CLASS).astype(np.float64)
    n_pat = conf.sum(axis=(1, 2))
    n, n1 = f["n"], f["n_y1"]
    n0 = n - n1
    out = {
        "n_patients": n_pat,
        "accuracy": _div0(f["correct"], n),
        "sensitivity": _div0(f["tp"], n1),
        "specificity": _div0(f["correct"] - f["tp"], n0),
        "overall_mean_variance": _div0(f["var_q"] / Q_SCALE, n),
        "mean_variance_class_0": _div0(f["var0_q"] / Q_SCALE, n0),
        "mean_variance_class_1": _div0(f["var1_q"] / Q_SCALE, n1),
        "mean_total_pred_entropy": _div0(f["ent_nats_q"] / Q_SCALE, n),
        "mean_expected_aleatoric_entropy": _div0(f["exp_ent_q"] / Q_SCALE, n),
        "mean_mutual_info": _div0(f["mi_q"] / Q_SCALE, n),
    }
    bias = _div0(f["err_q"] / Q_SCALE, n_pat)
    msq = _div0(f["sq_err_q"] / Q_SCALE, n_pat)
    var = np.where(n_pat > 1, np.maximum(msq - bias * bias, 0.0) * n_pat / np.where(n_pat > 1, n_pat - 1, 1), 0.0)
    sd = np.sqrt(var) * per_hour
    out["index_mae"] = _div0(f["abs_err_q"] / Q_SCALE, n_pat) * per_hour
    out["index_bias"] = bias * per_hour
    out["index_loa_lower"] = out["index_bias"] - 1.96 * sd
    out["index_loa_upper"] = out["index_bias"] + 1.96 * sd
    d = np.abs(np.arange(N_CLASS)[:, None] - np.arange(N_CLASS)[None, :])
    out["severity_accuracy"] = _div0((conf * (d == 0)).sum(axis=(1, 2)), n_pat)
    out["severity_within_one"] = _div0((conf * (d <= 1)).sum(axis=(1, 2)), n_pat)
    po = _div0((conf * KAPPA_W).sum(axis=(1, 2)), n_pat)
    row, col = conf.sum(axis=2), conf.sum(axis=1)
    pe = _div0(np.einsum("bi,ij,bj->b", row, KAPPA_W, col), n_pat * n_pat)
    out["severity_kappa_linear"] = np.where(pe < 1.0, (po - pe) / np.where(pe < 1.0, 1.0 - pe, 1.0), 0.0)
    out["ci_coverage"] = _div0(f["in_ci"], n_pat)
    out["share_confident"] = _div0(f["confident"], n_pat)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["severity_accuracy_confident"] = np.where(f["confident"] > 0,
                                                      f["confident_correct"] / np.where(f["confident"] > 0, f["confident"], 1),
                                                      np.nan)
    # Pearson r of patient accuracy and mean entropy: exact integer moments (Python ints cannot overflow)
    r = np.full(s.shape[0], np.nan)
    for b in range(s.shape[0]):
        k = int(s[b, N_PREC:].sum())
        sx, sy, sxx, syy, sxy = (int(s[b, COL[c]]) for c in ("acc_m", "ent_m", "acc2_m", "ent2_m", "accent_m"))
        dx, dy = k * sxx - sx * sx, k * syy - sy * sy
        if dx > 0 and dy > 0:
            r[b] = (k * sxy - sx * sy) / (np.sqrt(float(dx)) * np.sqrt(float(dy)))
    out["pearson_r_accuracy_entropy"] = r
    out["confusion"] = s[:, N_PREC:].reshape(-1, N_CLASS, N_CLASS).copy()
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out
