"""Pass / member-count convergence sums (``csrc/uq_converge.hip``) with an eager emulation.

``sums`` turns ``(T, n)`` probabilities, labels, ``(R, T)`` orders of the passes and ``K`` ascending counts
into ``(R, K, 11)`` int64: for order r and count k, the sums over the windows of the metrics of the subset
``probs[orders[r, :k]]``.  ``finalize`` is the only place where these integers become float64 means.  The
per-window values are fp64, quantised as ``rint(x 2^40)``; every sum over windows is an integer add, so the
result does not depend on the grid, on ``rep_groups``, on scheduling or on the sharding, and shards add
exactly.

Columns::

    0 n_valid   1 n_y1                                   windows with T finite probabilities; of these, y != 0
    2 var   3 var | y = 0   4 var | y = 1                ddof-0 variance max((k S2 - S1^2) / k^2, 0)
    5 H(mean)   6 E[H]   7 MI = max(H - E[H], 0)         nats, ``uq.metrics.binary_entropy_nats``
    8 correct   9 flips                                  label 2 S1 > k against y != 0 / against the label of all T
    10 |mean_k - mean_T|

``S1`` and ``S2`` are accumulated in fp64 in the order's sequence, and the all-T mean and label in the
order 0..T-1.  The kernel and the emulation add the same fp64 terms in the same sequence, so the integer
columns agree exactly; the quantised columns agree within one quantum per window (``log`` and the
contraction of ``k S2 - S1^2`` differ in the last bits between the two).  A pass's entropy enters ``E[H]`` as
the integer ``rint(h 2^52)``, so the entropy sum of a subset is exact in any order.  Two orders therefore
give the same k = T column when their ``S1`` and ``S2`` are exact (dyadic probabilities), and columns
within one quantum per window of each other otherwise.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _ext

# shared with the kernel (uq_converge.hip kCvScale / kCvMaxT / kCvCols and the binding's limits)
Q_BITS = 40
Q_SCALE = 1 << Q_BITS
ENT_BITS = 52                 # a pass's entropy (<= ln 2) as an integer: 128 of them stay below 2^59
ENT_SCALE = 1 << ENT_BITS
MAX_T = 128                   # 12 * 64 * T bytes of LDS per workgroup: 98,304 at T = 128
MAX_K = 32
MAX_R = 4096
MAX_N = 1 << 22               # per launch: a term is at most 2^40, so every sum stays below 2^62
TILE = 64                     # windows per workgroup
WAVES = 4                     # waves per workgroup = orders in flight per replicate group

COLS = ("n_valid", "n_y1", "var_q", "var0_q", "var1_q", "ent_q", "exp_ent_q", "mi_q", "correct", "flips", "shift_q")
N_COLS = len(COLS)
COL = {k: i for i, k in enumerate(COLS)}
INT_COLS = ("n_valid", "n_y1", "correct", "flips")
Q_COLS = tuple(c for c in COLS if c.endswith("_q"))
EPS = 1e-10

# the grid is ceil(n / 64) x rep_groups workgroups; LDS allows four of them per CU at T = 50
_CUS = 256
_FILL = 4 * _CUS


def _check(probs, y, orders, counts) -> Sequence[int]:
    if probs.dim() != 2:
        raise ValueError("probs must be (T, n)")
    t_count, n = probs.shape
    if not 1 <= t_count <= MAX_T:
        raise ValueError(f"T must be in 1..{MAX_T}")
    if n < 1:
        raise ValueError("no windows")
    if y.dim() != 1 or y.shape[0] != n:
        raise ValueError(f"y must be ({n},)")
    if orders.dim() != 2 or orders.shape[1] != t_count or not 1 <= orders.shape[0] <= MAX_R:
        raise ValueError(f"orders must be (R, {t_count}) with R in 1..{MAX_R}")
    srt = torch.sort(orders.long().cpu(), dim=1).values
    if not torch.equal(srt, torch.arange(t_count).expand_as(srt)):
        raise ValueError("every row of orders must be a permutation of 0..T-1")
    c = [int(v) for v in (counts.cpu().tolist() if isinstance(counts, torch.Tensor) else counts)]
    if not 1 <= len(c) <= MAX_K:
        raise ValueError(f"between 1 and {MAX_K} counts")
    if c[0] < 1 or c[-1] > t_count or any(b <= a for a, b in zip(c, c[1:])):
        raise ValueError(f"counts must be ascending values in 1..{t_count}")
    return c


def entropy_nats(p: torch.Tensor) -> torch.Tensor:
    """``uq.metrics.binary_entropy_nats`` in torch float64 (``cv_entropy`` of the kernel)."""
    pc, qc = p.clamp(EPS, 1 - EPS), (1 - p).clamp(EPS, 1 - EPS)
    s = pc + qc
    a, b = pc / s, qc / s
    return -(a * torch.log(a) + b * torch.log(b))


def quantise(x: torch.Tensor) -> torch.Tensor:
    """``cv_q`` of the kernel: rint(min(x, 1) 2^40) of a float64 value x >= 0.  No quantity of
    probabilities in [0, 1] exceeds 1; the clamp keeps a term at 2^40 for any other input."""
    return torch.round(x.clamp_max(1.0) * float(Q_SCALE)).long()


def sums_eager(probs: torch.Tensor, y: torch.Tensor, orders: torch.Tensor, counts,
               rep_groups: Optional[int] = None) -> torch.Tensor:
    """The arithmetic of ``converge_kernel`` in torch float64 / int64 (any device).  ``rep_groups`` is
    accepted for symmetry with :func:`sums` and changes nothing."""
    c = _check(probs, y, orders, counts)
    t_count = probs.shape[0]
    dev = probs.device
    ok = torch.isfinite(probs.float()).all(0)
    p_all = probs.float()[:, ok].double()
    y_all = (y.to(dev)[ok] != 0)
    od = orders.long().to(dev)
    n_rep = od.shape[0]
    out = torch.zeros(n_rep, len(c), N_COLS, dtype=torch.int64, device=dev)
    step = max(1, (1 << 20) // n_rep)   # R x step float64 accumulators at a time
    for lo in range(0, p_all.shape[1], step):
        p, y1 = p_all[:, lo:lo + step], y_all[lo:lo + step]
        h = torch.round(entropy_nats(p) * float(ENT_SCALE)).long()
        s_all = torch.zeros_like(p[0])
        for t in range(t_count):
            s_all = s_all + p[t]
        mean_all, lab_all = s_all / t_count, 2.0 * s_all > t_count
        m = p.shape[1]
        s1, s2 = (torch.zeros(n_rep, m, dtype=torch.float64, device=dev) for _ in range(2))
        sh = torch.zeros(n_rep, m, dtype=torch.int64, device=dev)
        kc = 0
        for i in range(t_count):
            pi = p[od[:, i]]
            s1 = s1 + pi
            s2 = s2 + pi * pi
            sh = sh + h[od[:, i]]
            if kc == len(c) or i + 1 != c[kc]:
                continue
            k = float(i + 1)
            mean = s1 / k
            vq = quantise(((k * s2 - s1 * s1) / (k * k)).clamp_min(0.0))
            ent, eh = entropy_nats(mean), sh.double() * (1.0 / ENT_SCALE) / k
            lab = 2.0 * s1 > k
            v1 = (vq * y1).sum(1)
            va = vq.sum(1)
            cols = [torch.full_like(va, m), torch.full_like(va, int(y1.sum())), va, va - v1, v1,
                    quantise(ent).sum(1), quantise(eh).sum(1), quantise((ent - eh).clamp_min(0.0)).sum(1),
                    (lab == y1).sum(1), (lab != lab_all).sum(1), quantise((mean - mean_all).abs()).sum(1)]
            out[:, kc] += torch.stack(cols, dim=1)
            kc += 1
    return out


def auto_rep_groups(n: int, n_rep: int) -> int:
    """Replicate groups of one launch over ``n`` windows.

    Every group stages the tile again (T loads and T fp64 entropies per window), so one group is the
    cheapest as soon as the ceil(n / 64) tiles alone fill the chip: four workgroups per CU, 1024 in all.
    Below that the orders are split until the grid reaches 1024 workgroups, at most into ceil(R / 4)
    groups (a group feeds four waves) and at most 8.  Measured on one MI355X at T = 50, 101 orders, ten
    counts (profiles/convergence_micro.json), rep_groups 1 / 2 / 4 / 8: 0.413 / 0.285 / 0.240 / 0.239 ms at
    16,384 windows (the rule picks 4), 1.46 / 1.41 / 1.42 / 1.53 ms at 131,072 and 10.31 / 10.47 / 10.92 /
    11.90 ms at 1,048,576 (the rule picks 1): the rule's choice is within 3.3 % of the best everywhere."""
    tiles = -(-n // TILE)
    g = 1
    while g < 8 and tiles * g < _FILL:
        g *= 2
    return max(1, min(g, -(-n_rep // WAVES)))


def sums(probs: torch.Tensor, y: torch.Tensor, orders: torch.Tensor, counts,
         rep_groups: Optional[int] = None) -> torch.Tensor:
    """(T, n) probabilities, (n,) labels, (R, T) orders, K ascending counts -> (R, K, 11) int64 sums.  The
    HIP kernel; everything must be on the GPU already or is moved there.  Sets above ``MAX_N`` windows are
    split and the parts added.  ``rep_groups`` (default :func:`auto_rep_groups`) only changes the speed."""
    c = _check(probs, y, orders, counts)
    if rep_groups is not None and not 1 <= int(rep_groups) <= 1024:
        raise ValueError("rep_groups must be in 1..1024")
    if not probs.is_cuda:
        raise ValueError("sums runs the HIP kernel: probs must be on the GPU (sums_eager is the emulation)")
    dev = probs.device
    p = probs.float().contiguous()
    yy = y.to(dev)
    od = orders.to(dev, torch.int32).contiguous()
    ct = torch.as_tensor(c, dtype=torch.int32, device=dev)
    n, n_rep = p.shape[1], od.shape[0]
    out = None
    for lo in range(0, n, MAX_N):
        hi = min(n, lo + MAX_N)
        g = auto_rep_groups(hi - lo, n_rep) if rep_groups is None else int(rep_groups)
        part = _ext.ops().converge(p if (lo, hi) == (0, n) else p[:, lo:hi].contiguous(), yy[lo:hi], od, ct, g)
        out = part if out is None else out + part
    return out


def _div0(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a / b with 0.0 where b == 0 (``metrics.class_mean``)."""
    return np.where(b > 0, a / np.where(b > 0, b, 1), 0.0)


def finalize(sums_) -> Dict[str, np.ndarray]:
    """(R, K, 11) (or (K, 11)) integer sums -> float64 means over the valid windows, one array per metric."""
    s = sums_.cpu().numpy() if isinstance(sums_, torch.Tensor) else np.asarray(sums_)
    if s.shape[-1] != N_COLS:
        raise ValueError(f"sums do not have {N_COLS} columns")
    f = {k: s[..., i].astype(np.float64) for k, i in COL.items()}
    n, n1 = f["n_valid"], f["n_y1"]
    n0 = n - n1
    return {
        "overall_mean_variance": _div0(f["var_q"] / Q_SCALE, n),
        "mean_variance_class_0": _div0(f["var0_q"] / Q_SCALE, n0),
        "mean_variance_class_1": _div0(f["var1_q"] / Q_SCALE, n1),
        "mean_total_pred_entropy": _div0(f["ent_q"] / Q_SCALE, n),
        "mean_expected_aleatoric_entropy": _div0(f["exp_ent_q"] / Q_SCALE, n),
        "mean_mutual_info": _div0(f["mi_q"] / Q_SCALE, n),
        "accuracy": _div0(f["correct"], n),
        "flip_rate": _div0(f["flips"], n),
        "mean_abs_shift": _div0(f["shift_q"] / Q_SCALE, n),
    }
