"""Recalibration kernels (``csrc/uq_recal.hip``) with torch float64 emulations that run anywhere.

``probs`` (T, n) fp32 is a prediction set, ``p_c = clip(p, 1e-7, 1 - 1e-7)`` (fp64 on the fp32 value),
``l1 = log p_c``, ``l0 = log1p(-p_c)``, ``f = (l1, -l0, 1)`` and ``theta = (a, b, c)`` maps every pass or member
to ``q_t = sigmoid(a l1_t - b l0_t + c)``.

``sums``   (F, Q, 12) fp64: ``n_valid, n_y1, loss, g_a, g_b, g_c, H_aa, H_ab, H_ac, H_bb, H_bc, H_cc`` over the valid
           windows (all T values finite, label 0 or 1, fold code in [0, F)) of fold g at candidate q, for the
           ``"joint"`` objective (the NLL of the pooled probability ``mean_t q_t``) or the ``"member"`` one (the
           mean over t of each pass's own NLL).  ``q`` and ``1 - q`` both come from ``e = exp(-|u|)``, the sum over
           t runs in the order 0..T-1 in the kernel and in :func:`sums_eager`; what differs between the two is the
           order of the fp64 additions over the windows, fused multiply-adds and a few ulps of ``exp`` / ``log``.
``apply``  (T, n) fp32, every window mapped by its fold's theta; NaN for a non-finite input or a bad fold code.

The kernel's result is bitwise independent of its launch grid and of how the candidates are split into calls:
the windows are cut into ranges of :func:`range_len` windows (a function of n only), a range is accumulated in
tile order into its own partial, the partials are added in range order, and a candidate's column is computed
without reference to its neighbours.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _ext
from .laplace import labels_u8

COLS = 12
COLUMNS = ("n_valid", "n_y1", "loss", "g_a", "g_b", "g_c", "H_aa", "H_ab", "H_ac", "H_bb", "H_bc", "H_cc")
OBJECTIVES = {"joint": 0, "member": 1}
EPS = 1e-7                   # the clip of golden_calibration's NLL
MAX_T, MAX_Q, MAX_F, MAX_N = 128, 64, 16, 1 << 27
TILE_WINDOWS = 64
MIN_RANGE = 256              # windows per range at least: four tiles
TARGET_RANGES = 256          # ranges aimed at (one per CU of an MI355X) where n allows
PARTIAL_LIMIT = 64 << 20     # bytes of range partials of one call
LDS_LIMIT = 160 * 1024
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def range_len(n: int) -> int:
    """Windows per range: n over 256 rounded up to the 64-window tile, at least 256.  Depends on n only."""
    need = -(-max(int(n), 1) // TARGET_RANGES)
    need = -(-need // TILE_WINDOWS) * TILE_WINDOWS
    return max(MIN_RANGE, need)


def n_ranges(n: int, rlen: Optional[int] = None) -> int:
    return -(-int(n) // int(rlen or range_len(n)))


def lds_bytes(T: int, F: int, Q: int) -> int:
    """LDS of one workgroup: the [T][2][64] fp64 planes, the (F, Q, 12) accumulator and the non-finite flags."""
    return T * 2 * TILE_WINDOWS * 8 + F * Q * COLS * 8 + 4 * TILE_WINDOWS * 4


def q_chunk(T: int, F: int, n: int, rlen: Optional[int] = None) -> int:
    """Candidates per launch: as many (64 at most) as keep the workgroup within 160 KiB of LDS and the range
    partials within 64 MB."""
    by_lds = (LDS_LIMIT - lds_bytes(T, F, 0)) // (F * COLS * 8)
    by_part = PARTIAL_LIMIT // (n_ranges(n, rlen) * F * COLS * 8)
    q = min(MAX_Q, by_lds, by_part)
    if q < 1:
        raise ValueError("no candidate fits the LDS / partial limits")
    return int(q)


def _objective(objective: Union[str, int]) -> int:
    if objective in OBJECTIVES:
        return OBJECTIVES[objective]
    if objective in (0, 1):
        return int(objective)
    raise ValueError(f"objective must be one of {tuple(OBJECTIVES)}")


def _fold(fold: Optional[torch.Tensor], n: int, F: int, device) -> torch.Tensor:
    if fold is None or fold.numel() == 0:
        if F != 1:
            raise ValueError("an empty fold needs n_folds = 1")
        return torch.empty(0, dtype=torch.int32, device=device)
    if fold.dim() != 1 or fold.numel() != n or fold.dtype != torch.int32:
        raise ValueError("fold must be (n,) int32")
    return fold.to(device)


def _check_sums(probs: torch.Tensor, y: torch.Tensor, thetas: torch.Tensor, F: int) -> None:
    if probs.dim() != 2 or probs.dtype != torch.float32:
        raise ValueError("probs must be (T, n) float32")
    T, n = probs.shape
    if not 1 <= T <= MAX_T:
        raise ValueError(f"T must be in 1..{MAX_T}")
    if not 1 <= n <= MAX_N:
        raise ValueError("n must be in 1..2^27")
    if thetas.dim() != 2 or thetas.shape[1] != 3 or thetas.dtype != torch.float64:
        raise ValueError("thetas must be (Q, 3) float64")
    if not 1 <= thetas.shape[0] <= MAX_Q:
        raise ValueError(f"Q must be in 1..{MAX_Q}")
    if not 1 <= int(F) <= MAX_F:
        raise ValueError(f"n_folds must be in 1..{MAX_F}")
    if y.numel() != n:
        raise ValueError(f"Mismatch between windows ({n}) and labels ({y.numel()})")


def planes_eager(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(l1, l0, finite)`` (T, n): fp64 logs of the clipped values (non-finite inputs read as 0.5)."""
    fin = torch.isfinite(probs)
    p = torch.where(fin, probs, torch.full_like(probs, 0.5)).double().clamp(EPS, 1.0 - EPS)
    return torch.log(p), torch.log1p(-p), fin


def _sigmoid_parts(u: torch.Tensor):
    """``q, 1 - q, q (1 - q), e`` from ``e = exp(-|u|)``."""
    e = torch.exp(-u.abs())
    inv = 1.0 / (1.0 + e)
    ei = e * inv
    pos = u >= 0
    return torch.where(pos, inv, ei), torch.where(pos, ei, inv), ei * inv, e


def sums_eager(probs: torch.Tensor, y: torch.Tensor, fold: Optional[torch.Tensor], thetas: torch.Tensor,
               n_folds: int = 1, objective: Union[str, int] = "joint", return_abs: bool = False):
    """:func:`sums` in torch float64 (any device).  ``return_abs``: also the (F, Q, 12) sums over the windows of
    the absolute inner terms of every float column (the counts as they are), from which a test bounds the
    rounding error of another order of additions."""
    F = int(n_folds)
    _check_sums(probs, y, thetas, F)
    obj = _objective(objective)
    dev = probs.device
    T, n = probs.shape
    Q = thetas.shape[0]
    fold = _fold(fold, n, F, dev)
    thetas = thetas.to(dev)
    y8 = labels_u8(y.to(dev))
    l1, l0, fin = planes_eager(probs)
    fc = fold.long() if fold.numel() else torch.zeros(n, dtype=torch.int64, device=dev)
    valid = fin.all(dim=0) & (y8 <= 1) & (fc >= 0) & (fc < F)
    y1 = y8 == 1
    a, b, c = (thetas[:, i][:, None] for i in range(3))
    z = torch.zeros(Q, n, dtype=torch.float64, device=dev)
    a0, a1 = z.clone(), z.clone()
    g = [z.clone() for _ in range(3)]
    h = [z.clone() for _ in range(6)]
    ga = [z.clone() for _ in range(3)]
    ha = [z.clone() for _ in range(6)]
    one = torch.ones(n, dtype=torch.float64, device=dev)
    for t in range(T):
        f = (l1[t], -l0[t], one)
        u = a * f[0] + b * f[1] + c
        q, o, s, e = _sigmoid_parts(u)
        if obj == 0:
            w = s * (o - q)
            a0 += q
            a1 += o
            gw, hw = s, w
        else:
            zz = torch.where(y1, -u, u)
            a0 += zz.clamp(min=0.0) + torch.log1p(e)
            gw, hw = torch.where(y1, -o, q), s
        for i in range(3):
            term = gw * f[i]
            g[i] += term
            ga[i] += term.abs()
        for k, (i, j) in enumerate(_PAIRS):
            term = hw * f[i] * f[j]
            h[k] += term
            ha[k] += term.abs()
    td = float(T)
    g = [v / td for v in g]
    h = [v / td for v in h]
    ga = [v / td for v in ga]
    ha = [v / td for v in ha]
    if obj == 0:
        pbar, obar = a0 / td, a1 / td
        hit = torch.where(y1, pbar, obar)
        miss = torch.where(y1, obar, pbar)
        r = torch.where(y1, -1.0 / hit, 1.0 / hit)
        k2 = r * r
        loss = torch.where(hit > 0.5, -torch.log1p(-miss), -torch.log(hit))
        cols = [loss] + [r * v for v in g] + [k2 * g[i] * g[j] + r * h[k] for k, (i, j) in enumerate(_PAIRS)]
        absc = [loss.abs()] + [r.abs() * v for v in ga] + [k2 * g[i].abs() * g[j].abs() + r.abs() * ha[k]
                                                           for k, (i, j) in enumerate(_PAIRS)]
    else:
        loss = a0 / td
        cols = [loss] + g + h
        absc = [loss.abs()] + ga + ha
    vd = valid.double()
    head = [vd.expand(Q, n), (valid & y1).double().expand(Q, n)]

    def reduce(columns):
        full = torch.stack(head + columns, dim=1)  # (Q, 12, n)
        out = torch.zeros(F, Q, COLS, dtype=torch.float64, device=dev)
        for fi in range(F):
            m = valid & (fc == fi)
            out[fi] = torch.where(m, full, torch.zeros_like(full)).sum(dim=2)
        return out

    out = reduce(cols)
    return (out, reduce(absc)) if return_abs else out


def sums(probs: torch.Tensor, y: torch.Tensor, fold: Optional[torch.Tensor], thetas: torch.Tensor, n_folds: int = 1,
         objective: Union[str, int] = "joint", grid: int = 0, rlen: Optional[int] = None,
         chunk: Optional[int] = None) -> torch.Tensor:
    """(F, Q, 12) fp64 on ``probs``'s device: the HIP kernel on the GPU, else the torch emulation.  ``grid``
    (workgroups; 0 = one per range), ``rlen`` (windows per range; None = :func:`range_len`) and ``chunk``
    (candidates per launch; None = :func:`q_chunk`) are test hooks: the result depends on ``rlen`` only."""
    F = int(n_folds)
    _check_sums(probs, y, thetas, F)
    obj = _objective(objective)
    if not probs.is_cuda:
        return sums_eager(probs, y, fold, thetas, F, obj)
    dev = probs.device
    T, n = probs.shape
    rl = int(rlen or range_len(n))
    qc = q_chunk(T, F, n, rl)
    if chunk is not None:
        if not 1 <= int(chunk) <= qc:
            raise ValueError(f"chunk must be in 1..{qc} for this T, n_folds and n")
        qc = int(chunk)
    fold = _fold(fold, n, F, dev)
    y8 = labels_u8(y.to(dev))
    pp = probs.contiguous()
    th = thetas.to(dev).contiguous()
    op = _ext.ops().recal_sums
    outs = [op(pp, y8, fold, th[s:s + qc].contiguous(), F, obj, rl, int(grid)) for s in range(0, th.shape[0], qc)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


def _check_apply(probs: torch.Tensor, thetas: torch.Tensor) -> None:
    if probs.dim() != 2 or probs.dtype != torch.float32:
        raise ValueError("probs must be (T, n) float32")
    if thetas.dim() != 2 or thetas.shape[1] != 3 or thetas.dtype != torch.float64:
        raise ValueError("thetas must be (F, 3) float64")
    if not 1 <= thetas.shape[0] <= MAX_F:
        raise ValueError(f"F must be in 1..{MAX_F}")


def apply_eager(probs: torch.Tensor, fold: Optional[torch.Tensor], thetas: torch.Tensor) -> torch.Tensor:
    """:func:`apply` in torch float64 (any device), rounded once to fp32."""
    _check_apply(probs, thetas)
    dev = probs.device
    n = probs.shape[1]
    F = thetas.shape[0]
    fold = _fold(fold, n, F, dev)
    thetas = thetas.to(dev)
    fc = fold.long() if fold.numel() else torch.zeros(n, dtype=torch.int64, device=dev)
    ok = (fc >= 0) & (fc < F)
    th = thetas[torch.where(ok, fc, torch.zeros_like(fc))]  # (n, 3)
    l1, l0, fin = planes_eager(probs)
    u = th[:, 0] * l1 - th[:, 1] * l0 + th[:, 2]
    q = _sigmoid_parts(u)[0].float()
    return torch.where(fin & ok[None], q, torch.full_like(q, float("nan")))


def apply(probs: torch.Tensor, fold: Optional[torch.Tensor], thetas: torch.Tensor) -> torch.Tensor:
    """(T, n) fp32 ``sigmoid(a l1 - b l0 + c)`` with ``(a, b, c) = thetas[fold]``: the HIP kernel on the GPU, else
    :func:`apply_eager`."""
    _check_apply(probs, thetas)
    if not probs.is_cuda:
        return apply_eager(probs, fold, thetas)
    fold = _fold(fold, probs.shape[1], thetas.shape[0], probs.device)
    return _ext.ops().recal_apply(probs.contiguous(), fold, thetas.to(probs.device).contiguous())
