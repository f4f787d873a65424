"""Ensemble-composition sums (``csrc/uq_members.hip``) with an eager emulation.

``pairs`` turns ``(T, n)`` probabilities and labels into the symmetric ``(T, T, 3)`` int64 pair table and the
header ``(n_valid, n_y1)``; ``mix`` turns them, optional fold codes and ``(Q, T)`` integer member counts into
``(F, Q, 7)`` int64 sums of the mixtures ``sum_t c_t p_t / k``.  ``finalize_pairs`` and ``finalize_mix`` are
the only places where these integers become float64.

Pair table, with ``r_t = (double)p_t - (y != 0)`` and ``c_t`` = "member t is correct" (label ``p > 0.5``)::

    0 both_y0   sum_w [c_a and c_b and y = 0]        the diagonal holds the member's true negatives,
    1 both_y1   sum_w [c_a and c_b and y = 1]        its true positives
    2 gram_q    sum_w rint(r_a r_b 2^40)             and n x Brier

Mixture sums, with ``s = sum_t c_t p_t`` accumulated in fp64 in the order t = 0..T-1 and ``m = s / k``::

    0 n_valid   1 n_y1      windows with T finite probabilities; of these, y != 0
    2 nll_q                 sum rint(nll 2^36), nll = -log(clip(m or 1 - m, 1e-7, 1 - 1e-7))
    3 brier_q               sum rint((m - y)^2 2^40)
    4 correct   5 true_pos   6 pred_pos     label 2 s > k

The subtraction ``p - y``, the product ``r_a r_b``, the division ``s / k``, ``m - y`` and its square are single
correctly rounded fp64 operations, ``c_t p_t`` and the scalings by a power of two are exact, and every sum
over windows is an integer add.  The kernel and the emulation therefore give the same integers in every column
but ``nll_q``, which is within one quantum per valid window (``log`` differs in its last bits), for any grid,
any order of the windows and any sharding; shards add exactly.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _ext

# shared with the kernels (uq_members.hip kMb* and the binding's limits)
BRIER_BITS = 40
BRIER_SCALE = 1 << BRIER_BITS
NLL_BITS = 36                 # nll <= 16.12 < 2^5: a term stays below 2^41
NLL_SCALE = 1 << NLL_BITS
CLIP = 1e-7                   # the NLL clip of uq/calibration.py and uq/recalibration.py
MAX_T = 128
MAX_Q = 64                    # rows per launch; ``mix`` chunks more
MAX_F = 16
MAX_COUNT = 255
MAX_N_PAIRS = 1 << 22         # per launch: a term is at most 2^40, so every sum stays below 2^62
MAX_N_MIX = 1 << 21           # per launch: an nll term stays below 2^41
TILE = 64

PAIR_COLS = ("both_y0", "both_y1", "gram_q")
MIX_COLS = ("n_valid", "n_y1", "nll_q", "brier_q", "correct", "true_pos", "pred_pos")
N_MIX_COLS = len(MIX_COLS)
MIX = {k: i for i, k in enumerate(MIX_COLS)}
PAIR_STATS = ("disagreement", "double_fault", "q_statistic", "error_correlation", "kappa")


def _check_probs(probs, y) -> None:
    if probs.dim() != 2:
        raise ValueError("probs must be (T, n)")
    t_count, n = probs.shape
    if not 1 <= t_count <= MAX_T:
        raise ValueError(f"T must be in 1..{MAX_T}")
    if n < 1:
        raise ValueError("no windows")
    if y.dim() != 1 or y.shape[0] != n:
        raise ValueError(f"y must be ({n},)")


def _check_mix(probs, y, counts, fold, n_folds: int) -> torch.Tensor:
    """The counts as a (Q, T) int64 CPU tensor, after every check that needs values."""
    _check_probs(probs, y)
    t_count, n = probs.shape
    c = torch.as_tensor(np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts)).long()
    if c.dim() != 2 or c.shape[1] != t_count or c.shape[0] < 1:
        raise ValueError(f"counts must be (Q, {t_count}) with Q >= 1")
    if int(c.min()) < 0 or int(c.max()) > MAX_COUNT:
        raise ValueError(f"counts must lie in 0..{MAX_COUNT}")
    if int(c.sum(1).min()) < 1:
        raise ValueError("every row of counts needs a positive sum")
    if not 1 <= int(n_folds) <= MAX_F:
        raise ValueError(f"n_folds must be in 1..{MAX_F}")
    if fold is not None:
        if fold.dim() != 1 or fold.shape[0] != n:
            raise ValueError(f"fold must be ({n},)")
        if int(fold.min()) < 0 or int(fold.max()) >= int(n_folds):
            raise ValueError(f"fold codes must lie in 0..{int(n_folds) - 1}")
    return c


def _rint_q(x: torch.Tensor, scale: int) -> torch.Tensor:
    """rint(x scale) as int64, round to nearest even (``mb_rint`` of the kernel)."""
    return torch.round(x * float(scale)).long()


# ===================== member_pairs =====================
def pairs_eager(probs: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The arithmetic of ``member_pairs_kernel`` in torch float64 / int64 (any device): the (T, T, 3) table and
    the (2,) header."""
    _check_probs(probs, y)
    dev = probs.device
    t_count = probs.shape[0]
    pf = probs.float()
    ok = torch.isfinite(pf).all(0)
    p_all, y_all = pf[:, ok], (y.to(dev)[ok] != 0)
    table = torch.zeros(t_count, t_count, 3, dtype=torch.int64, device=dev)
    head = torch.tensor([int(ok.sum()), int(y_all.sum())], dtype=torch.int64, device=dev)
    step = max(1, (1 << 22) // (t_count * t_count))   # T x T x step float64 products at a time
    for lo in range(0, p_all.shape[1], step):
        p, y1 = p_all[:, lo:lo + step], y_all[lo:lo + step]
        r = (p.double() - y1.double()).clamp(-1.0, 1.0)   # |r| <= 1 for probabilities; the clamp bounds a term
        c = (p > 0.5) == y1
        c0, c1 = (c & ~y1).double(), (c & y1).double()   # 0 / 1 products and their sums are exact in float64
        table[..., 0] += (c0 @ c0.T).long()
        table[..., 1] += (c1 @ c1.T).long()
        table[..., 2] += _rint_q(r[:, None, :] * r[None, :, :], BRIER_SCALE).sum(-1)
    return table, head


def pairs(probs: torch.Tensor, y: torch.Tensor, grid: Optional[int] = None,
          slices: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(T, n) probabilities and (n,) labels -> the (T, T, 3) int64 pair table and the (2,) header.  The HIP
    kernel; ``probs`` must be on the GPU.  Sets above ``MAX_N_PAIRS`` windows are split and the parts added.
    ``grid`` (workgroups that share the 64-window tiles) and ``slices`` (threads per 4 x 4 patch of the pair
    matrix, a power of two up to 64) default to the launcher's choice and only change the speed."""
    _check_probs(probs, y)
    if grid is not None and not 1 <= int(grid) <= 65535:
        raise ValueError("grid must be in 1..65535")
    if slices is not None and (not 1 <= int(slices) <= 64 or int(slices) & (int(slices) - 1)):
        raise ValueError("slices must be a power of two in 1..64")
    if not probs.is_cuda:
        raise ValueError("pairs runs the HIP kernel: probs must be on the GPU (pairs_eager is the emulation)")
    p = probs.float().contiguous()
    yy = (y.to(p.device) != 0).to(torch.int32).contiguous()
    n = p.shape[1]
    table = head = None
    for lo in range(0, n, MAX_N_PAIRS):
        hi = min(n, lo + MAX_N_PAIRS)
        t, h = _ext.ops().member_pairs(p if (lo, hi) == (0, n) else p[:, lo:hi].contiguous(), yy[lo:hi].contiguous(),
                                       int(grid or 0), int(slices or 0))
        table, head = (t, h) if table is None else (table + t, head + h)
    return table, head


# ===================== member_mix =====================
def mix_eager(probs: torch.Tensor, y: torch.Tensor, counts, fold: Optional[torch.Tensor] = None,
              n_folds: int = 1) -> torch.Tensor:
    """The arithmetic of ``member_mix_kernel`` in torch float64 / int64 (any device): (F, Q, 7) int64."""
    c = _check_mix(probs, y, counts, fold, n_folds)
    dev = probs.device
    t_count, n_rows, n_f = probs.shape[0], c.shape[0], int(n_folds)
    pf = probs.float()
    ok = torch.isfinite(pf).all(0)
    p_all, y_all = pf[:, ok].double(), (y.to(dev)[ok] != 0)
    f_all = torch.zeros_like(y_all, dtype=torch.int64) if fold is None else fold.to(dev)[ok].long()
    cd = c.to(dev).double()
    k = c.sum(1).to(dev).double()[:, None]
    out = torch.zeros(n_f, n_rows, N_MIX_COLS, dtype=torch.int64, device=dev)
    step = max(1, (1 << 21) // n_rows)   # Q x step float64 accumulators at a time
    for lo in range(0, p_all.shape[1], step):
        p, y1, fo = p_all[:, lo:lo + step], y_all[lo:lo + step], f_all[lo:lo + step]
        s = torch.zeros(n_rows, p.shape[1], dtype=torch.float64, device=dev)
        for t in range(t_count):
            s = s + cd[:, t, None] * p[t]   # c_t p_t is exact; a zero count adds 0.0
        m = s / k
        lab = 2.0 * s > k
        pt = torch.where(y1, m, 1.0 - m)
        nll_q = _rint_q(-torch.log(pt.clamp(CLIP, 1.0 - CLIP)), NLL_SCALE)
        d = m - y1.double()
        brier_q = _rint_q((d * d).clamp_max(1.0), BRIER_SCALE)   # <= 1 for probabilities; the clamp bounds a term
        one = torch.ones_like(nll_q)
        cols = torch.stack([one, one * y1, nll_q, brier_q, (lab == y1).long(), (lab & y1).long(), lab.long()], dim=-1)
        for f in range(n_f):
            out[f] += (cols * (fo == f)[None, :, None]).sum(1)
    return out


def mix(probs: torch.Tensor, y: torch.Tensor, counts, fold: Optional[torch.Tensor] = None, n_folds: int = 1,
        grid: Optional[int] = None) -> torch.Tensor:
    """(T, n) probabilities, (n,) labels, (Q, T) integer counts and optional (n,) fold codes -> (F, Q, 7) int64.
    The HIP kernel; ``probs`` must be on the GPU.  Rows are chunked by ``MAX_Q`` (they are independent, so a
    row's result does not depend on its chunk) and sets above ``MAX_N_MIX`` windows are split and the parts
    added.  ``grid`` (workgroups that share the 64-window tiles) only changes the speed."""
    c = _check_mix(probs, y, counts, fold, n_folds)
    if grid is not None and not 1 <= int(grid) <= 65535:
        raise ValueError("grid must be in 1..65535")
    if not probs.is_cuda:
        raise ValueError("mix runs the HIP kernel: probs must be on the GPU (mix_eager is the emulation)")
    p = probs.float().contiguous()
    dev = p.device
    yy = (y.to(dev) != 0).to(torch.int32).contiguous()
    fd = None if fold is None else fold.to(dev, torch.uint8).contiguous()
    cc = c.to(torch.int32).contiguous()   # a host tensor: the binding checks its values and uploads it with the launch
    n = p.shape[1]
    out = None
    for lo in range(0, n, MAX_N_MIX):
        hi = min(n, lo + MAX_N_MIX)
        whole = (lo, hi) == (0, n)
        pp, ys = (p, yy) if whole else (p[:, lo:hi].contiguous(), yy[lo:hi].contiguous())
        fs = fd if whole or fd is None else fd[lo:hi].contiguous()
        part = torch.cat([_ext.ops().member_mix(pp, ys, fs, cc[q:q + MAX_Q].contiguous(), int(n_folds), int(grid or 0))
                          for q in range(0, cc.shape[0], MAX_Q)], dim=1)
        out = part if out is None else out + part
    return out


# ===================== integers -> float64 =====================
def _np(a) -> np.ndarray:
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _div(a, b):
    """a / b in float64, NaN where b == 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    zero = b == 0
    return np.where(zero, np.nan, a / np.where(zero, 1.0, b))


def _pair_stats(correct: np.ndarray, both: np.ndarray, pos: np.ndarray, n: float) -> Dict[str, np.ndarray]:
    """The count-based pair statistics from, per member, the correct windows and the windows labelled positive,
    per pair the windows where both are correct, and the number of windows."""
    ca, cb = correct[:, None], correct[None, :]
    n11 = both
    n10, n01 = ca - n11, cb - n11           # a right and b wrong; a wrong and b right
    n00 = n - ca - cb + n11
    cross = n11 * n00 - n01 * n10
    po = _div(n11 + n00, n)                 # two labels: agreeing on the label = agreeing on correctness
    pa, pb = pos[:, None], pos[None, :]
    pe = _div(pa * pb + (n - pa) * (n - pb), n * n)
    return {"disagreement": _div(n10 + n01, n), "double_fault": _div(n00, n),
            "q_statistic": _div(cross, n11 * n00 + n01 * n10),
            "error_correlation": _div(cross, np.sqrt(ca * (n - ca) * cb * (n - cb))),
            "kappa": _div(po - pe, 1.0 - pe)}


def finalize_pairs(table, head) -> Dict[str, np.ndarray]:
    """The (T, T, 3) table and the header -> float64 (T, T) matrices: ``disagreement``, ``double_fault``,
    ``q_statistic``, ``error_correlation`` (the phi coefficient of the correctness table), ``kappa`` (Cohen's, of
    the two label vectors), each also restricted to the windows of one class (``_y0`` / ``_y1``), and
    ``residual_correlation``; NaN where a denominator is 0.  Also ``n_valid``, ``n_y1``, the per-member counts
    ``true_neg``, ``true_pos``, ``pred_pos`` and ``gram`` = the residual Gram in float64 (sums of r_a r_b)."""
    t = _np(table).astype(np.float64)
    h = _np(head).astype(np.float64)
    if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
        raise ValueError("the pair table must be (T, T, 3)")
    n, n1 = float(h[0]), float(h[1])
    n0 = n - n1
    tn, tp = np.diagonal(t[..., 0]).copy(), np.diagonal(t[..., 1]).copy()
    out = {"n_valid": n, "n_y1": n1, "true_neg": tn, "true_pos": tp, "pred_pos": tp + n0 - tn,
           "gram": t[..., 2] / BRIER_SCALE}
    out.update(_pair_stats(tn + tp, t[..., 0] + t[..., 1], out["pred_pos"], n))
    for suffix, cnt, both, pos, nc in (("_y0", tn, t[..., 0], n0 - tn, n0), ("_y1", tp, t[..., 1], tp, n1)):
        out.update({k + suffix: v for k, v in _pair_stats(cnt, both, pos, nc).items()})
    g = np.diagonal(t[..., 2])
    out["residual_correlation"] = _div(t[..., 2], np.sqrt(g[:, None] * g[None, :]))
    return out


def finalize_mix(sums_) -> Dict[str, np.ndarray]:
    """(..., 7) integer sums -> float64 ``nll``, ``brier``, ``accuracy``, ``sensitivity``, ``specificity`` (means
    over the valid windows; NaN where there are none) and ``n_valid``."""
    s = _np(sums_)
    if s.shape[-1] != N_MIX_COLS:
        raise ValueError(f"sums do not have {N_MIX_COLS} columns")
    f = {k: s[..., i].astype(np.float64) for k, i in MIX.items()}
    n, n1 = f["n_valid"], f["n_y1"]
    return {"n_valid": n, "nll": _div(f["nll_q"] / NLL_SCALE, n), "brier": _div(f["brier_q"] / BRIER_SCALE, n),
            "accuracy": _div(f["correct"], n), "sensitivity": _div(f["true_pos"], n1),
            "specificity": _div(f["correct"] - f["true_pos"], n - n1)}
