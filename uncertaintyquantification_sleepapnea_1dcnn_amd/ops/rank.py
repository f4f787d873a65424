"""Rank statistics of bootstrap replicates from one sort (``csrc/uq_rank.hip``) with a bit-compatible eager emulation.

Resampling does not change the order of the scores.  ``prep`` sorts the windows once and packs, per sorted
window, the binary target and the tie-group-start flag into one byte (plain torch: it runs once per call,
not per replicate).  A replicate is then a row of integer weights over the sorted windows (``weights``:
the multiplicity of each window among the draws; ``cluster_weights``: the multiplicity of its patient), and
``scan_sums`` turns weight rows into (B, 6) int64 sums ``W, P, U2, groups, prauc_q, ap_q``; ``finalize``
is the only place where integers become float64.

With ``P_g``, ``N_g`` the weighted positives / negatives of tie group g in ascending score order::

    U2      = sum_g P_g (2 cumN_before_g + N_g)            twice the Mann-Whitney U
    prauc_q = sum_g rint(2^56 dR_g (prec_g + prec_prev_g) / 2)
    ap_q    = sum_g rint(2^56 dR_g prec_g)

over the groups of non-zero weight, with ``TP_g = P - cumP_before_g``, ``FP_g = N - cumN_before_g``,
``prec_g = TP_g / (TP_g + FP_g)``, ``prec_prev_g`` the precision of the next higher non-empty group (1 for
the highest) and ``dR_g = P_g / P``.  Every sum is an integer sum, so the result does not depend on the
launch grid.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _ext
from .rng import boot_row

COLS = ("W", "P", "U2", "groups", "prauc_q", "ap_q")
W_COL, P_COL, U2_COL, GROUPS_COL, PRAUC_COL, AP_COL = range(6)
# fixed-point scale of the PR terms (uq_rank.hip kRankQScale): a term is quantised to rint(term 2^S) before
# it is added, an error of at most n 2^-(S+1) = 2^-30 < 1e-9 at n = 2^27; the terms add up to at most 1, so
# the sums stay at 2^56, far below 2^63
S_BITS = 56
Q_SCALE = float(1 << S_BITS)
MAX_N = 1 << 27              # sorted windows
MAX_W = 1 << 31              # a replicate's total weight stays below: U2 <= W^2 / 2 < 2^61
MAX_SPLITS = 64              # uq_rank.hip kRankMaxSplits
Z_BIT, START_BIT = 1, 2      # packed byte: target, first window of a tie group
# the weight rows of a chunk of replicates stay within this many bytes (one row where a row alone is larger:
# 2^27 windows are 512 MB); bootstrap_sums loops over chunks
WORKSPACE_BYTES = 256 << 20

# automatic split count (measured in profiles/rank_micro.json at B = 100): B * G stays within TARGET_BLOCKS
# workgroups and a split has at least MIN_SPLIT_WINDOWS sorted windows; G is a power of two
TARGET_BLOCKS = 2048
MIN_SPLIT_WINDOWS = 8192


def auto_splits(n: int, n_boot: int) -> int:
    """Splits G per replicate: the largest power of two within TARGET_BLOCKS / B, n / MIN_SPLIT_WINDOWS and 64."""
    g = max(1, min(TARGET_BLOCKS // max(n_boot, 1), n // MIN_SPLIT_WINDOWS, MAX_SPLITS))
    return 1 << (g.bit_length() - 1)


def chunk_replicates(n: int) -> int:
    """Replicates per chunk: as many weight rows (n rounded up to 4 int32) as fit WORKSPACE_BYTES, at least 1."""
    return max(1, WORKSPACE_BYTES // (4 * ((n + 3) // 4 * 4)))


def prep(score: torch.Tensor, target: torch.Tensor) -> Dict:
    """Sort once.  ``score`` (n,) floating, ``target`` (n,) (non-zero = positive) on one device.

    Windows with a non-finite score are dropped.  Returns ``perm`` (n_valid,) int64, the window at every
    sorted position (ascending score); ``pos`` (n,) int32, the sorted position of every window (-1:
    dropped); ``packed`` (n_valid,) uint8, ``target | group_start << 1`` per sorted window; ``sorted``
    (the sorted scores), ``n_valid`` and ``n_total``."""
    s = score.reshape(-1)
    if not s.is_floating_point() or s.dtype in (torch.float16, torch.bfloat16):
        s = s.float()
    n_total = s.numel()
    if target.numel() != n_total:
        raise ValueError(f"Mismatch between scores ({n_total}) and targets ({target.numel()})")
    valid = torch.nonzero(torch.isfinite(s)).reshape(-1)
    n = valid.numel()
    if n > MAX_N:
        raise ValueError(f"at most {MAX_N} windows")
    srt, order = torch.sort(s[valid], stable=True)
    perm = valid[order]
    pos = torch.full((n_total,), -1, dtype=torch.int32, device=s.device)
    pos[perm] = torch.arange(n, dtype=torch.int32, device=s.device)
    z = (target.reshape(-1).to(s.device)[perm] != 0)
    start = torch.ones(n, dtype=torch.bool, device=s.device)
    if n > 1:
        start[1:] = srt[1:] != srt[:-1]
    packed = (z.to(torch.uint8) * Z_BIT) | (start.to(torch.uint8) * START_BIT)
    return {"perm": perm, "pos": pos, "packed": packed, "sorted": srt, "n_valid": int(n), "n_total": int(n_total)}


def split_bounds(packed: torch.Tensor, splits: int) -> torch.Tensor:
    """(G + 1,) int32 split points: ``g n / G`` moved down to the start of its tie group, so that no group
    straddles a split (a group longer than a split leaves splits empty)."""
    n = packed.numel()
    if not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"splits must be in 1..{MAX_SPLITS}")
    dev = packed.device
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    is_start = (packed & START_BIT) != 0
    if n:
        is_start = is_start.clone()
        is_start[0] = True
    group_start = torch.cummax(torch.where(is_start, ar, torch.zeros_like(ar)), 0).values if n else ar
    nominal = (torch.arange(splits, dtype=torch.int64, device=dev) * n) // splits
    b = group_start[nominal] if n else nominal
    return torch.cat([b, torch.full((1,), n, dtype=torch.int64, device=dev)]).to(torch.int32)


def _check_draws(pos: torch.Tensor, n_sorted: int) -> None:
    if pos.numel() > MAX_N:
        raise ValueError(f"at most {MAX_N} windows")
    if not 0 <= n_sorted <= pos.numel():
        raise ValueError("n_sorted must be in 0..len(pos)")


def weights_eager(pos: torch.Tensor, n_sorted: int, n_boot: int, idx: Optional[torch.Tensor] = None, seed: int = 0,
                  b0: int = 0) -> torch.Tensor:
    """(B, n_sorted) int32 of ``rank_count_kernel`` in torch: row b counts how often every sorted window is
    drawn by replicate ``b0 + b`` (``idx[b]``, else the counter hash).  Draws outside [0, n) and draws of
    dropped windows are skipped."""
    _check_draws(pos, n_sorted)
    n, dev = pos.numel(), pos.device
    out = torch.zeros(n_boot, n_sorted, dtype=torch.int32, device=dev)
    p = pos.long()
    for b in range(n_boot):
        draws = boot_row(n, b0 + b, seed, dev) if idx is None else idx[b].long().to(dev)
        k = p[draws[(draws >= 0) & (draws < n)]]
        k = k[(k >= 0) & (k < n_sorted)]
        out[b] = torch.bincount(k, minlength=n_sorted).to(torch.int32)
    return out


def weights(pos: torch.Tensor, n_sorted: int, n_boot: int, idx: Optional[torch.Tensor] = None, seed: int = 0,
            b0: int = 0) -> torch.Tensor:
    """Weight rows of replicates ``b0 .. b0 + B - 1``: the HIP kernel on the GPU (rows on 16-B boundaries),
    else :func:`weights_eager`.  ``idx`` (B, n) holds these replicates' draws."""
    _check_draws(pos, n_sorted)
    seed = int(seed) & 0xFFFFFFFF
    if pos.is_cuda and n_sorted > 0 and n_boot > 0:
        return _ext.ops().rank_count(pos, None if idx is None else idx.to(pos.device), seed, int(b0), int(n_boot),
                                     int(n_sorted))
    return weights_eager(pos, n_sorted, n_boot, idx, seed, b0)


def cluster_weights(mult: torch.Tensor, code_sorted: torch.Tensor) -> torch.Tensor:
    """(B, n_sorted) int32 weights of the patient-cluster bootstrap: ``mult[b, code_sorted]``, the number of
    times replicate b drew the patient of every sorted window.  A torch gather, no atomics (rows on 16-B
    boundaries for the scan kernel)."""
    n = code_sorted.numel()
    buf = torch.zeros(mult.shape[0], (n + 3) // 4 * 4, dtype=torch.int32, device=mult.device)
    w = buf[:, :n]
    w.copy_(torch.index_select(mult.to(torch.int32), 1, code_sorted.long()))
    return w


def multiplicities(draws: torch.Tensor, n_pat: int) -> torch.Tensor:
    """(B, P) int32: how often every patient occurs in each row of ``draws`` (B, P'); values outside [0, P) are skipped."""
    d = draws.long()
    ok = (d >= 0) & (d < n_pat)
    out = torch.zeros(d.shape[0], n_pat, dtype=torch.int32, device=d.device)
    out.scatter_add_(1, torch.where(ok, d, torch.zeros_like(d)), ok.to(torch.int32))
    return out


def _check_scan(w: torch.Tensor, packed: torch.Tensor) -> None:
    if w.dim() != 2 or w.dtype != torch.int32:
        raise ValueError("w must be (B, n) int32")
    if packed.dim() != 1 or packed.dtype != torch.uint8 or packed.numel() != w.shape[1]:
        raise ValueError("packed must be (n,) uint8")
    if w.shape[1] > MAX_N:
        raise ValueError(f"at most {MAX_N} windows")


def scan_sums_eager(w: torch.Tensor, packed: torch.Tensor) -> torch.Tensor:
    """(B, 6) int64 sums of ``rank_totals_kernel`` + ``rank_scan_kernel`` in torch int64 / float64 (any device)."""
    _check_scan(w, packed)
    n_boot, n = w.shape
    dev = w.device
    out = torch.zeros(n_boot, len(COLS), dtype=torch.int64, device=dev)
    if n == 0 or n_boot == 0:
        return out
    if int(w.min()) < 0:
        raise ValueError("weights must be non-negative")
    wl = w.long()
    z = (packed & Z_BIT).long()
    start = (packed & START_BIT) != 0
    start = start.clone()
    start[0] = True
    gid = torch.cumsum(start.long(), 0) - 1
    n_groups = int(gid[-1]) + 1
    pg = torch.zeros(n_boot, n_groups, dtype=torch.int64, device=dev).index_add_(1, gid, wl * z)
    ng = torch.zeros(n_boot, n_groups, dtype=torch.int64, device=dev).index_add_(1, gid, wl * (1 - z))
    p_tot, n_tot = pg.sum(1, keepdim=True), ng.sum(1, keepdim=True)
    if int((p_tot + n_tot).max()) >= MAX_W:
        raise ValueError("a replicate's total weight must stay below 2^31")
    p_before = torch.cumsum(pg, 1) - pg
    n_before = torch.cumsum(ng, 1) - ng
    has = (pg + ng) > 0
    tp, fp = p_tot - p_before, n_tot - n_before          # at or above the group's score
    tp_prev, fp_prev = tp - pg, fp - ng                  # strictly above
    one = torch.ones((), dtype=torch.float64, device=dev)
    prec = tp.double() / torch.where(has, tp + fp, torch.ones_like(tp)).double()
    above = (tp_prev + fp_prev) > 0
    prec_prev = torch.where(above, tp_prev.double() / torch.where(above, tp_prev + fp_prev, torch.ones_like(tp)).double(), one)
    d_recall = pg.double() / torch.where(p_tot > 0, p_tot, torch.ones_like(p_tot)).double()
    use = has & (pg > 0)
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    pr_q = torch.where(use, torch.round(d_recall * (prec + prec_prev) * 0.5 * Q_SCALE).long(), zero)
    ap_q = torch.where(use, torch.round(d_recall * prec * Q_SCALE).long(), zero)
    out[:, W_COL] = (p_tot + n_tot)[:, 0]
    out[:, P_COL] = p_tot[:, 0]
    out[:, U2_COL] = (pg * (2 * n_before + ng)).sum(1)
    out[:, GROUPS_COL] = has.sum(1)
    out[:, PRAUC_COL] = pr_q.sum(1)
    out[:, AP_COL] = ap_q.sum(1)
    return out


def scan_sums(w: torch.Tensor, packed: torch.Tensor, splits: int = 0, bounds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, 6) int64 sums ``COLS`` of the weight rows ``w`` (B, n) int32 over the sorted windows.  ``splits`` =
    G of the launch grid (0 = automatic); the result does not depend on it."""
    _check_scan(w, packed)
    if w.is_cuda and w.shape[0] > 0 and w.shape[1] > 0:
        if bounds is None:
            bounds = split_bounds(packed, int(splits) or auto_splits(w.shape[1], w.shape[0]))
        try:
            return _ext.ops().rank_scan(w, packed, bounds)
        except RuntimeError as e:
            if "rank_scan:" in str(e) and ("2^31" in str(e) or "non-negative" in str(e)):
                raise ValueError(str(e).split("\n")[0]) from None
            raise
    return scan_sums_eager(w, packed)


def bootstrap_sums(pr: Dict, n_boot: int, idx: Optional[torch.Tensor] = None, seed: int = 0, splits: int = 0,
                   mult: Optional[torch.Tensor] = None, code: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, 6) int64 sums of B replicates of a :func:`prep` result, in chunks of :func:`chunk_replicates`.

    Window bootstrap: ``idx`` (B, n_total) draws, else the counter hash with ``seed``.  Patient-cluster
    bootstrap: ``mult`` (B, P) int32 patient multiplicities and ``code`` (n_total,) the patient of every
    window."""
    n = pr["n_valid"]
    dev = pr["packed"].device
    out = torch.zeros(n_boot, len(COLS), dtype=torch.int64, device=dev)
    if n == 0 or n_boot == 0:
        return out
    bounds = split_bounds(pr["packed"], int(splits) or auto_splits(n, min(n_boot, chunk_replicates(n)))) \
        if pr["packed"].is_cuda else None
    code_sorted = None if mult is None else code.to(dev).long()[pr["perm"]]
    step = chunk_replicates(n)
    for b0 in range(0, n_boot, step):
        b1 = min(n_boot, b0 + step)
        if mult is not None:
            w = cluster_weights(mult[b0:b1].to(dev), code_sorted)
        else:
            w = weights(pr["pos"], n, b1 - b0, None if idx is None else idx[b0:b1], seed, b0)
        out[b0:b1] = scan_sums(w, pr["packed"], bounds=bounds)
    return out


def check_cluster_limit(n_pat: int, max_size: int) -> None:
    """A replicate draws P patients; were all of them the largest, its weight must still stay below 2^31."""
    if n_pat * max_size >= MAX_W:
        raise ValueError(f"patients ({n_pat}) x largest patient ({max_size} windows) must stay below 2^31")


def finalize(sums) -> Dict[str, np.ndarray]:
    """(B, 6) or (6,) integer sums -> float64 ``auroc = U2 / (2 P N)``, ``pr_auc``, ``average_precision``,
    ``u_statistic = U2 / 2`` and the integers ``n_pos``, ``n_neg``, ``groups``.  The three ratios are NaN
    for a replicate without positives or without negatives."""
    s = sums.cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    single = s.ndim == 1
    s = np.atleast_2d(s).astype(np.int64)
    if s.shape[1] != len(COLS):
        raise ValueError(f"sums do not have {len(COLS)} columns")
    p = s[:, P_COL]
    n = s[:, W_COL] - p
    both = (p > 0) & (n > 0)
    den = np.where(both, 2 * p * n, 1).astype(np.float64)  # 2 P N < 2^63 in integers, then one rounding
    nan = np.full(len(s), np.nan)
    out = {
        "auroc": np.where(both, s[:, U2_COL].astype(np.float64) / den, nan),
        "pr_auc": np.where(both, s[:, PRAUC_COL].astype(np.float64) / Q_SCALE, nan),
        "average_precision": np.where(both, s[:, AP_COL].astype(np.float64) / Q_SCALE, nan),
        "u_statistic": s[:, U2_COL].astype(np.float64) / 2.0,
        "n_pos": p.copy(), "n_neg": n.copy(), "groups": s[:, GROUPS_COL].copy(),
    }
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out
