"""Calibration / selective-prediction sums (``csrc/uq_calib.hip``) with a bit-compatible eager emulation.

``prep`` turns each window's mean probability, uncertainty score and label into one (4,) int32 record
``[p_q, code, brier_q, nll_q]``; ``bootstrap_sums`` gathers the records of every bootstrap draw and
returns (B, S) int64 raw sums, ``S = 3 K + 4 (J + 1) + 2``; ``finalize`` turns sums into float64
metrics.  Everything between ``prep`` and ``finalize`` is integer arithmetic, so the sums do not depend
on the launch grid, on scheduling or on how the windows are sharded, and sums of shards are exact.

Column layout of the sums (K confidence bins, J thresholds)::

    [3 k + {0, 1, 2}]           bin k: count, positives, sum p_q
    [3 K + 4 u + {0, 1, 2, 3}]  uncertainty bucket u (0..J): count, correct, positives, true positives
    [S - 2], [S - 1]            sum brier_q, sum nll_q
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _ext
from .rng import boot_row

# fixed-point scales shared with the kernels (uq_calib.hip kCalibPScale / kCalibNllScale)
P_BITS = 30
NLL_BITS = 27
P_SCALE = 1 << P_BITS        # p_q = rint(p * 2^30), brier_q = rint((p - y)^2 * 2^30)
NLL_SCALE = 1 << NLL_BITS    # nll_q = rint(nll * 2^27); nll <= -log(1e-7) = 16.2 fits 32 unsigned bits
NLL_EPS = 1e-7               # Keras binary cross-entropy epsilon
MAX_BINS = 32
MAX_THR = 64
MAX_N = 1 << 27              # keeps sum nll_q below 2^63

# code word: conf_bin | unc_bucket << 5 | y << 12 | pred << 13 | correct << 14
BUCKET_SHIFT, Y_SHIFT, PRED_SHIFT, CORRECT_SHIFT = 5, 12, 13, 14

# multi-slice grid (measured in profiles/calib_micro.json at B = 100): G is a power of two, because slice
# counts that leave a partial second round of workgroups measure slower (G = 3 is behind G = 2 and G = 4
# at every size); B * G stays within TARGET_BLOCKS, beyond which more slices gain nothing; and a slice has
# at least MIN_SLICE_DRAWS draws: from 16,384 windows on G = 2 is about 15 % faster than G = 1, at 8,192
# the two are within 3 %
TARGET_BLOCKS = 512
MIN_SLICE_DRAWS = 8192


def n_columns(n_bins: int, n_thr: int) -> int:
    return 3 * n_bins + 4 * (n_thr + 1) + 2


def auto_slices(n_global: int, n_boot: int) -> int:
    """Slices G per replicate: the largest power of two within TARGET_BLOCKS / B and n / MIN_SLICE_DRAWS."""
    g = max(1, min(TARGET_BLOCKS // max(n_boot, 1), n_global // MIN_SLICE_DRAWS, 1024))
    return 1 << (g.bit_length() - 1)


def _check(n: int, n_bins: int, n_thr: int) -> None:
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"n_bins must be in 1..{MAX_BINS}")
    if not 0 <= n_thr <= MAX_THR:
        raise ValueError(f"at most {MAX_THR} thresholds")
    if n > MAX_N:
        raise ValueError(f"at most {MAX_N} windows")


def unpack(rec: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Fields of (N, 4) int32 records as int64 tensors."""
    r = rec.long()
    code = r[:, 1]
    return {"p_q": r[:, 0], "conf_bin": code & 31, "unc_bucket": (code >> BUCKET_SHIFT) & 127,
            "y": (code >> Y_SHIFT) & 1, "pred": (code >> PRED_SHIFT) & 1, "correct": (code >> CORRECT_SHIFT) & 1,
            "brier_q": r[:, 2], "nll_q": r[:, 3] & 0xFFFFFFFF}


def prep_eager(p: torch.Tensor, score: torch.Tensor, y: torch.Tensor, thr: torch.Tensor, n_bins: int) -> torch.Tensor:
    """The integer arithmetic of ``calib_prep_kernel`` in torch (any device)."""
    _check(p.numel(), n_bins, thr.numel())
    pf = torch.nan_to_num(p.float(), nan=0.0).clamp(0.0, 1.0)
    pd = pf.double()
    yy = (y != 0).long()
    p_q = torch.round(pd * P_SCALE).long()
    conf_bin = ((p_q * n_bins) >> P_BITS).clamp_max(n_bins - 1)
    sc = score.float()
    bucket = torch.searchsorted(thr.float().contiguous(), sc.contiguous(), right=False)  # #{j : thr[j] < score}
    bucket = torch.where(torch.isnan(sc), torch.zeros_like(bucket), bucket).long()
    pred = (pf > 0.5).long()
    correct = (pred == yy).long()
    brier_q = torch.round((pd - yy.double()) ** 2 * P_SCALE).long()
    pt = pd.clamp(NLL_EPS, 1.0 - NLL_EPS)
    nll = -torch.log(torch.where(yy == 1, pt, 1.0 - pt))
    nll_q = torch.round(nll * NLL_SCALE).long()
    nll_q = torch.where(nll_q >= (1 << 31), nll_q - (1 << 32), nll_q)  # unsigned 32 bits in an int32 word
    code = conf_bin | (bucket << BUCKET_SHIFT) | (yy << Y_SHIFT) | (pred << PRED_SHIFT) | (correct << CORRECT_SHIFT)
    return torch.stack([p_q, code, brier_q, nll_q], dim=1).to(torch.int32)


def prep(p: torch.Tensor, score: torch.Tensor, y: torch.Tensor, thr: torch.Tensor, n_bins: int) -> torch.Tensor:
    """(N,) mean probability, (N,) score, (N,) labels, (J,) sorted thresholds -> (N, 4) int32 records."""
    _check(p.numel(), n_bins, thr.numel())
    if p.is_cuda:
        dev = p.device
        return _ext.ops().calib_prep(p.float().contiguous(), score.to(dev).float().contiguous(), y.to(dev),
                                     thr.to(dev).float().contiguous(), int(n_bins))
    return prep_eager(p, score, y, thr, n_bins)


def _hash_row(n: int, b: int, seed: int, device) -> torch.Tensor:
    """Row b of ``ops.uq._hash_idx(n, B, seed)`` without the other rows."""
    return boot_row(n, b, seed, device)


def bootstrap_sums_eager(rec: torch.Tensor, idx: Optional[torch.Tensor], seed: int, n_boot: int, n_global: int,
                         lo: int, n_bins: int, n_thr: int) -> torch.Tensor:
    """(B, S) int64 sums of ``calib_bootstrap_kernel`` in torch: draws of replicate b that land in
    windows [lo, lo + len(rec)) are gathered and histogrammed with exact int64 adds."""
    n_loc = rec.shape[0]
    _check(n_global, n_bins, n_thr)
    dev = rec.device
    f = unpack(rec)
    conf_bin = f["conf_bin"].clamp_max(n_bins - 1)
    bucket = f["unc_bucket"].clamp_max(n_thr)
    tp = f["y"] * f["pred"]
    one = torch.ones(n_loc, dtype=torch.int64, device=dev)
    conf_src = torch.stack([one, f["y"], f["p_q"]], dim=1)
    buck_src = torch.stack([one, f["correct"], f["y"], tp], dim=1)
    tot_src = torch.stack([f["brier_q"], f["nll_q"]], dim=1)
    out = torch.zeros(n_boot, n_columns(n_bins, n_thr), dtype=torch.int64, device=dev)
    for b in range(n_boot):
        draws = _hash_row(n_global, b, seed, dev) if idx is None else idx[b].long()
        k = draws - lo
        k = k[(draws >= 0) & (draws < n_global) & (k >= 0) & (k < n_loc)]
        conf = torch.zeros(n_bins, 3, dtype=torch.int64, device=dev).index_add_(0, conf_bin[k], conf_src[k])
        buck = torch.zeros(n_thr + 1, 4, dtype=torch.int64, device=dev).index_add_(0, bucket[k], buck_src[k])
        out[b] = torch.cat([conf.reshape(-1), buck.reshape(-1), tot_src[k].sum(0)])
    return out


def bootstrap_sums(rec: torch.Tensor, n_boot: int, n_bins: int, n_thr: int, idx: Optional[torch.Tensor] = None,
                   seed: int = 0, n_global: Optional[int] = None, lo: int = 0, slices: int = 0) -> torch.Tensor:
    """(B, S) int64 raw sums over the draws landing in this shard's windows [lo, lo + len(rec)) of
    ``n_global`` (default: unsharded).  ``idx`` (B, n_global) gives the draws, else the counter hash of
    ``ops.uq.bootstrap`` with the same ``seed``.  ``slices`` = G of the launch grid (0 = automatic);
    the result does not depend on it.  Sum the shards' results, then :func:`finalize`."""
    n_global = rec.shape[0] if n_global is None else int(n_global)
    _check(n_global, n_bins, n_thr)
    seed = int(seed) & 0xFFFFFFFF
    if rec.is_cuda:
        g = int(slices) or auto_slices(n_global, n_boot)
        return _ext.ops().calib_bootstrap(rec, None if idx is None else idx.to(rec.device), seed, int(n_boot), n_global,
                                          int(lo), int(n_bins), int(n_thr), g)
    return bootstrap_sums_eager(rec, idx, seed, n_boot, n_global, lo, n_bins, n_thr)


def _div(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a / b with NaN where b == 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, a / np.where(b > 0, b, 1), np.nan)


def aurc(coverage: np.ndarray, accuracy: np.ndarray) -> float:
    """Area under the risk-coverage curve: trapezoid of 1 - accuracy over coverage, non-NaN points."""
    ok = ~(np.isnan(coverage) | np.isnan(accuracy))
    c, r = np.asarray(coverage)[ok], 1.0 - np.asarray(accuracy)[ok]
    if c.size < 2:
        return float("nan") if c.size == 0 else 0.0
    return float(np.sum(0.5 * (r[1:] + r[:-1]) * (c[1:] - c[:-1])))


def finalize(sums, n_draws: int, n_bins: int, n_thr: int) -> Dict[str, np.ndarray]:
    """(B, S) or (S,) integer sums -> float64 metrics (arrays with a leading B axis for 2-D input).

    ``bin_confidence = sum p_q / (2^30 count)``, ``bin_frequency = positives / count``; ``ece`` weighs
    ``|frequency - confidence|`` by ``count / n`` (empty bins add 0), ``mce`` is its maximum over the
    non-empty bins; per threshold j the prefix sums over buckets 0..j give coverage, accuracy,
    sensitivity and specificity (NaN on a zero denominator); ``aurc`` as :func:`aurc`."""
    s = sums.cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    single = s.ndim == 1
    s = np.atleast_2d(s).astype(np.int64)
    if s.shape[1] != n_columns(n_bins, n_thr):
        raise ValueError("sums do not have 3 K + 4 (J + 1) + 2 columns")
    n_draws = float(n_draws)
    conf = s[:, :3 * n_bins].reshape(-1, n_bins, 3)
    buck = s[:, 3 * n_bins:3 * n_bins + 4 * (n_thr + 1)].reshape(-1, n_thr + 1, 4)
    count = conf[:, :, 0].astype(np.float64)
    confidence = _div(conf[:, :, 2].astype(np.float64) / P_SCALE, count)
    frequency = _div(conf[:, :, 1].astype(np.float64), count)
    gap = np.abs(frequency - confidence)
    has = count > 0
    ece = np.sum(np.where(has, count / n_draws * np.where(has, gap, 0.0), 0.0), axis=1)
    mce = np.where(has.any(axis=1), np.max(np.where(has, gap, -np.inf), axis=1), np.nan)
    pre = np.cumsum(buck, axis=1)[:, :n_thr, :].astype(np.float64)  # threshold j retains buckets 0..j
    kept, corr, pos, tpos = pre[:, :, 0], pre[:, :, 1], pre[:, :, 2], pre[:, :, 3]
    neg = kept - pos
    tneg = corr - tpos
    out = {
        "bin_count": conf[:, :, 0].copy(),
        "bin_confidence": confidence,
        "bin_frequency": frequency,
        "ece": ece,
        "mce": mce,
        "brier": s[:, -2].astype(np.float64) / P_SCALE / n_draws,
        "nll": s[:, -1].astype(np.float64) / NLL_SCALE / n_draws,
        "coverage": kept / n_draws,
        "accuracy": _div(corr, kept),
        "sensitivity": _div(tpos, pos),
        "specificity": _div(tneg, neg),
    }
    out["aurc"] = np.array([aurc(c, a) for c, a in zip(out["coverage"], out["accuracy"])])
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out
