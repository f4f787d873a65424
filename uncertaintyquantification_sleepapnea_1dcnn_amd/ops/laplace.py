"""Last-layer Laplace kernels (``csrc/uq_laplace.hip``) with torch float64 emulations that run anywhere.

``phi`` (n, D) fp32 are the penultimate features, ``phi~ = [phi; 1]``, ``theta`` (D + 1,) fp64 the dense head
(kernel, then bias).  All arithmetic is fp64 on the fp32 feature values.

``gram``     the fit-set sums: ``H = sum_i w_i phi~_i phi~_i^T`` with ``w_i = p_i (1 - p_i)``,
             ``g = sum_i (p_i - y_i) phi~_i``, ``loglik`` and ``n_valid`` over the valid windows (every feature
             finite, label 0 or 1).  The logit ``f_i`` is formed the same way by the kernel and by
             :func:`logits_eager` (four partial sums over the features c = j mod 4 in ascending order,
             multiply and add rounded separately, then ``((a0 + a1) + (a2 + a3)) + bias``), so both see the same
             bits of ``f_i``; ``w_i = e / (1 + e)^2`` with ``e = exp(-|f_i|)`` keeps its relative accuracy where
             ``1 - p`` would cancel.  What differs between the kernel and the emulation is the order of the
             fp64 additions over the windows and a few ulps of ``exp`` / ``log1p``.
``predict``  ``Phi~ [theta | M]`` with ``M = [theta_1 .. theta_T | L]``: sample probabilities (T, n) fp32, the
             mean logit ``mu``, the logit variance ``v = |L^T phi~|^2`` and the probit-corrected probability.

The Gram kernel's result is bitwise independent of its launch grid: the windows are cut into ranges of
:func:`range_len` windows (a function of n and D only), a range is accumulated in window order into its
own partial, and the partials are added in range order.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, Optional, Tuple

import torch

from . import _ext

MAX_D1 = 128                 # uq_laplace.hip kLapMaxDP: D + 1, padded to a multiple of 16
TILE_WINDOWS = 64            # windows staged in LDS at a time
COL_BLOCK = 64               # columns of [theta | M] staged in LDS at a time
PARTIAL_LIMIT = 64 << 20     # bytes of range partials of one Gram call
MIN_RANGE = 256              # windows per range at least: four tiles
TARGET_RANGES = 256          # ranges aimed at (one per CU of an MI355X) where n allows

_warned = set()


def padded(D: int) -> int:
    """D + 1 rounded up to the MFMA tile (16)."""
    return (D + 1 + 15) // 16 * 16


def supports(D: int) -> bool:
    return 1 <= D and D + 1 <= MAX_D1


def warn_unsupported(D: int, what: str) -> None:
    """One warning per D: the HIP kernels hold D + 1 <= 128 features; wider heads run the torch float64 path."""
    if D not in _warned:
        _warned.add(D)
        warnings.warn(f"last-layer Laplace {what}: no HIP kernel for D + 1 = {D + 1} > {MAX_D1}; "
                      "running the torch float64 formulation", RuntimeWarning, stacklevel=3)


def partial_doubles(D: int) -> int:
    """fp64 values of one range's partial: H (padded), g (padded), loglik, n_valid."""
    dp = padded(D)
    return dp * dp + dp + 2


def range_len(n: int, D: int) -> int:
    """Windows per range: n over TARGET_RANGES rounded up to the 64-window tile, at least MIN_RANGE, and as many
    more as keep the partials of all ranges within PARTIAL_LIMIT.  Depends on n and D only."""
    max_ranges = max(1, min(TARGET_RANGES, PARTIAL_LIMIT // (8 * partial_doubles(D))))
    need = -(-max(int(n), 1) // max_ranges)
    need = -(-need // TILE_WINDOWS) * TILE_WINDOWS
    return max(MIN_RANGE, need)


def n_ranges(n: int, D: int, rlen: Optional[int] = None) -> int:
    return -(-int(n) // int(rlen or range_len(n, D)))


def bytes_partial(n: int, D: int, rlen: Optional[int] = None) -> int:
    """Bytes of the range partials of a Gram call over n windows."""
    return n_ranges(n, D, rlen) * partial_doubles(D) * 8


def col_blocks(D: int, T: int) -> int:
    """Column blocks of [theta | theta_1 .. theta_T | L] the predict kernel stages in LDS."""
    return -(-(1 + int(T) + D + 1) // COL_BLOCK)


def labels_u8(y: torch.Tensor) -> torch.Tensor:
    """Labels as uint8: 0, 1, or 2 for anything else (invalid)."""
    y = y.reshape(-1)
    two = torch.full_like(y, 2, dtype=torch.uint8)
    return torch.where(y == 0, torch.zeros_like(two), torch.where(y == 1, torch.ones_like(two), two))


def flat_size(D: int) -> int:
    return (D + 1) * (D + 1) + (D + 1) + 2


def unflatten(flat: torch.Tensor, D: int) -> Dict[str, torch.Tensor]:
    """[H | g | loglik | n_valid] -> dict (views)."""
    d1 = D + 1
    return {"H": flat[: d1 * d1].view(d1, d1), "g": flat[d1 * d1: d1 * d1 + d1], "loglik": flat[d1 * d1 + d1],
            "n_valid": flat[d1 * d1 + d1 + 1]}


def _check_gram(phi: torch.Tensor, theta: torch.Tensor, y: torch.Tensor) -> None:
    if phi.dim() != 2 or phi.dtype != torch.float32 or phi.shape[1] < 1:
        raise ValueError("phi must be (n, D) float32")
    if theta.dim() != 1 or theta.dtype != torch.float64 or theta.numel() != phi.shape[1] + 1:
        raise ValueError("theta must be (D + 1,) float64")
    if y.numel() != phi.shape[0]:
        raise ValueError(f"Mismatch between features ({phi.shape[0]}) and labels ({y.numel()})")


def logits_eager(x64: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """``f = theta . [x; 1]`` in the kernel's order of operations (bit-compatible)."""
    D = x64.shape[1]
    xt = x64.t().contiguous()
    a = [torch.zeros(x64.shape[0], dtype=torch.float64, device=x64.device) for _ in range(4)]
    for c in range(D):
        a[c % 4] = a[c % 4] + theta[c] * xt[c]
    return ((a[0] + a[1]) + (a[2] + a[3])) + theta[D]


def gram_flat_eager(phi: torch.Tensor, theta: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The flat [H | g | loglik | n_valid] of :func:`gram` in torch float64 (any device)."""
    _check_gram(phi, theta, y)
    y8 = labels_u8(y.to(phi.device))
    x = phi.double()
    valid = torch.isfinite(x).all(dim=1) & (y8 <= 1)
    x = torch.where(valid[:, None], x, torch.zeros_like(x))
    f = logits_eager(x, theta)
    e = torch.exp(-f.abs())
    inv = 1.0 / (1.0 + e)
    pos = f >= 0
    p = torch.where(pos, inv, e * inv)
    q = torch.where(pos, e * inv, inv)
    vd = valid.double()
    one = y8 == 1
    w = e * inv * inv * vd
    r = torch.where(one, -q, p) * vd
    z = torch.where(one, -f, f)
    ll = -(z.clamp(min=0.0) + torch.log1p(e)) * vd
    xt = torch.cat([x, vd[:, None]], dim=1)
    H = (xt * w[:, None]).t() @ xt
    H = torch.triu(H) + torch.triu(H, 1).t()
    g = xt.t() @ r
    return torch.cat([H.reshape(-1), g, ll.sum().reshape(1), vd.sum().reshape(1)])


def gram_flat(phi: torch.Tensor, theta: torch.Tensor, y: torch.Tensor, grid: int = 0,
              rlen: Optional[int] = None) -> torch.Tensor:
    """Flat fp64 [H | g | loglik | n_valid] on ``phi``'s device: the HIP kernel on the GPU, else the torch
    emulation.  ``grid`` (workgroups; 0 = one per range) and ``rlen`` (windows per range; None =
    :func:`range_len`) are test hooks: the result does not depend on ``grid``."""
    _check_gram(phi, theta, y)
    D = phi.shape[1]
    if phi.is_cuda and supports(D):
        n = phi.shape[0]
        rl = int(rlen or range_len(n, D))
        if bytes_partial(n, D, rl) > PARTIAL_LIMIT:
            raise ValueError("the range partials must stay within 64 MB")
        return _ext.ops().laplace_gram(phi, theta.to(phi.device), labels_u8(y.to(phi.device)), rl, int(grid))
    if phi.is_cuda:
        warn_unsupported(D, "fit")
    return gram_flat_eager(phi, theta.to(phi.device), y)


def _as_dict(flat: torch.Tensor, D: int, n_total: int) -> Dict:
    d = unflatten(flat, D)
    return {"H": d["H"], "g": d["g"], "loglik": float(d["loglik"]), "n_valid": int(round(float(d["n_valid"]))),
            "n_total": int(n_total)}


def gram(phi: torch.Tensor, theta: torch.Tensor, y: torch.Tensor, grid: int = 0, rlen: Optional[int] = None) -> Dict:
    """``{"H" (D+1, D+1), "g" (D+1,), "loglik", "n_valid", "n_total"}`` of the fit set (fp64 tensors, Python scalars)."""
    return _as_dict(gram_flat(phi, theta, y, grid, rlen), phi.shape[1], phi.shape[0])


def gram_eager(phi: torch.Tensor, theta: torch.Tensor, y: torch.Tensor) -> Dict:
    return _as_dict(gram_flat_eager(phi, theta, y), phi.shape[1], phi.shape[0])


def _check_predict(phi: torch.Tensor, M: torch.Tensor, theta: torch.Tensor, T: int) -> None:
    if phi.dim() != 2 or phi.dtype != torch.float32 or phi.shape[1] < 1:
        raise ValueError("phi must be (n, D) float32")
    d1 = phi.shape[1] + 1
    if theta.dim() != 1 or theta.dtype != torch.float64 or theta.numel() != d1:
        raise ValueError("theta must be (D + 1,) float64")
    if T < 0 or M.dim() != 2 or M.dtype != torch.float64 or tuple(M.shape) != (d1, T + d1):
        raise ValueError("M must be (D + 1, T + D + 1) float64: [theta_1 .. theta_T | L]")


def _sigmoid64(x: torch.Tensor) -> torch.Tensor:
    e = torch.exp(-x.abs())
    inv = 1.0 / (1.0 + e)
    return torch.where(x >= 0, inv, e * inv)


def predict_eager(phi: torch.Tensor, M: torch.Tensor, theta: torch.Tensor, T: int,
                  return_logits: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(preds (T, n) fp32, mu, v, probit (n,) fp64)`` in torch float64 (any device); ``return_logits``: the
    sample logits (T, n) fp64 in place of the probabilities."""
    _check_predict(phi, M, theta, T)
    x = phi.double()
    bad = ~torch.isfinite(x).all(dim=1)
    x = torch.where(bad[:, None], torch.zeros_like(x), x)
    xt = torch.cat([x, torch.ones(x.shape[0], 1, dtype=torch.float64, device=x.device)], dim=1)
    out = xt @ torch.cat([theta[:, None], M], dim=1)
    mu = out[:, 0]
    v = (out[:, 1 + T:] ** 2).sum(dim=1)
    probit = _sigmoid64(mu / torch.sqrt(1.0 + (math.pi / 8.0) * v))
    lg = out[:, 1: 1 + T].t()
    preds = lg.contiguous() if return_logits else _sigmoid64(lg).float().contiguous()
    nan = float("nan")
    preds[:, bad] = nan
    mu, v, probit = (torch.where(bad, torch.full_like(t, nan), t) for t in (mu, v, probit))
    return preds, mu, v, probit


def predict(phi: torch.Tensor, M: torch.Tensor, theta: torch.Tensor,
            T: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Sample probabilities and logit moments: the HIP kernel on the GPU, else :func:`predict_eager`."""
    _check_predict(phi, M, theta, T)
    D = phi.shape[1]
    if phi.is_cuda and supports(D):
        mx = torch.cat([theta[:, None], M], dim=1).to(phi.device).contiguous()
        preds, mom = _ext.ops().laplace_predict(phi, mx, int(T))
        return preds, mom[0], mom[1], mom[2]
    if phi.is_cuda:
        warn_unsupported(D, "predict")
    return predict_eager(phi, M.to(phi.device), theta.to(phi.device), T)
