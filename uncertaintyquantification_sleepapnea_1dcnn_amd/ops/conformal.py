"""Split conformal prediction over random calibration / test splits (``csrc/uq_conformal.hip``) with a
bit-compatible eager emulation.

The windows are sorted once (``ops/rank.py:prep``); a split is a role per sorted window.  The role is a pure
function of ``(seed, split r, unit u)`` (``ops/rng.py:split_hash``), evaluated where it is needed, so no
``(R, n)`` array exists::

    unit u calibrates in split r  iff  split_hash(seed, r, u) < cal_thr,   cal_thr = floor(cal_fraction 2^32)
    pooled:     every window of a calibrating unit calibrates, every other window is a test window
    subsample:  of a calibrating unit only the window with within == (split_hash2(seed, r, u) ucount[u]) >> 32
                calibrates; its other windows are neither calibration nor test

``select`` returns per split the totals ``cal0, cal1, test0, test1`` and, per stratum and miscoverage level, the
sorted position of the calibration window of rank ``k(n_cal)`` (:func:`rank_k`); ``count`` the test windows of
either class below a cut.  :func:`assemble` turns prefix counts at the two cuts ``e0`` (sorted windows with label
0 in the set) and ``s1`` (sorted windows with label 1 *not* in the set) into the integer counts ``COLS`` and
:func:`finalize` is the only place where integers become float64.  Everything before it is integer, so nothing
depends on the launch (``segments``).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _ext
from .rng import split_hash, split_hash2

PPM = 10 ** 6
MAX_N = 1 << 27          # sorted windows
MAX_ALPHA = 32           # uq_conformal.hip kConfMaxAlpha
MAX_CUTS = 64            # kConfMaxCuts
TILE = 512               # kConfTile: windows per wave step
MAX_SEGMENTS = 4096      # kConfMaxSeg
Z_BIT = 1                # packed byte: the class, as ops/rank.py writes it
# per class z: test windows, those with label 0 / label 1 in the set, with both, with neither
COLS = tuple(f"{c}_{z}" for z in (0, 1) for c in ("n_test", "incl0", "incl1", "both", "empty"))
METRICS = ("coverage", "coverage_class_0", "coverage_class_1", "share_empty", "share_singleton", "share_both",
           "mean_set_size", "singleton_accuracy")


def alpha_to_ppm(alphas) -> np.ndarray:
    """``round(alpha 10^6)`` as int64; every level must land in 1..999,999."""
    a = np.atleast_1d(np.asarray(alphas, np.float64))
    ppm = np.rint(np.where(np.isfinite(a), a, 0.0) * PPM).astype(np.int64)
    if a.size == 0 or ppm.min() < 1 or ppm.max() > PPM - 1:
        raise ValueError("miscoverage levels must lie in [1e-6, 1 - 1e-6]")
    return ppm


def rank_k(n, alpha_ppm):
    """``k(n) = ceil((n + 1)(1 - alpha))`` in integers: ``((n + 1)(10^6 - alpha_ppm) + 10^6 - 1) // 10^6`` (int64;
    NumPy arrays, torch tensors or ints, broadcast).  ``k > n`` means an infinite threshold."""
    return ((n + 1) * (PPM - alpha_ppm) + PPM - 1) // PPM


def cal_threshold(cal_fraction: float) -> int:
    """``floor(cal_fraction 2^32)`` in [0, 2^32]."""
    f = float(cal_fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError("cal_fraction must lie in [0, 1]")
    return int(np.floor(f * 4294967296.0))


def _check_roles(unit, packed, within, ucount, cal_thr, r0, n_splits) -> None:
    if unit.dim() != 1 or unit.dtype != torch.int32:
        raise ValueError("unit must be (n,) int32")
    n = unit.numel()
    if n > MAX_N:
        raise ValueError(f"at most {MAX_N} windows")
    if packed.dim() != 1 or packed.dtype != torch.uint8 or packed.numel() != n:
        raise ValueError("packed must be (n,) uint8")
    if (within is None) != (ucount is None):
        raise ValueError("within and ucount go together")
    if within is not None:
        if within.dim() != 1 or within.dtype != torch.int32 or within.numel() != n:
            raise ValueError("within must be (n,) int32")
        if ucount.dim() != 1 or ucount.dtype != torch.int32 or ucount.numel() < 1:
            raise ValueError("ucount must be (P,) int32")
    if not 0 <= int(cal_thr) <= 1 << 32:
        raise ValueError("cal_thr must be in 0..2^32")
    if n_splits < 0 or r0 < 0 or r0 + n_splits >= 1 << 31:
        raise ValueError("bad split range")


def roles_eager(seed: int, r: int, unit: torch.Tensor, within: Optional[torch.Tensor], ucount: Optional[torch.Tensor],
                cal_thr: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(calibrates, tests)`` bool tensors over the windows of ``unit`` in split ``r``.  A unit outside
    ``ucount`` counts as empty (its pick is window 0), as in the kernel."""
    seed = int(seed) & 0xFFFFFFFF
    u = unit.long()
    cal_unit = split_hash(seed, r, u) < int(cal_thr)
    cal = cal_unit
    if within is not None:
        inside = (u >= 0) & (u < ucount.numel())
        cnt = torch.where(inside, ucount.long()[torch.where(inside, u, torch.zeros_like(u))] & 0xFFFFFFFF,
                          torch.zeros_like(u))
        pick = (split_hash2(seed, r, u) * cnt) >> 32
        # the kernel compares the int32 within against the pick as int32
        pick = torch.where(pick >= 1 << 31, pick - (1 << 32), pick)
        cal = cal_unit & (within.long() == pick)
    return cal, ~cal_unit


def select_eager(unit: torch.Tensor, packed: torch.Tensor, within: Optional[torch.Tensor], ucount: Optional[torch.Tensor],
                 seed: int, r0: int, n_splits: int, cal_thr: int, alpha_ppm: torch.Tensor,
                 strata: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``conformal_select_kernel`` in torch (any device), one split at a time."""
    _check_roles(unit, packed, within, ucount, cal_thr, r0, n_splits)
    if strata not in (1, 2):
        raise ValueError("strata must be 1 or 2")
    n_alpha = alpha_ppm.numel()
    if not 1 <= n_alpha <= MAX_ALPHA:
        raise ValueError(f"1..{MAX_ALPHA} miscoverage levels")
    dev = unit.device
    ppm = alpha_ppm.long().to(dev).clamp(1, PPM - 1)
    z = (packed & Z_BIT) != 0
    totals = torch.zeros(n_splits, 4, dtype=torch.int32, device=dev)
    member = torch.full((n_splits, strata, n_alpha), -1, dtype=torch.int32, device=dev)
    if unit.numel() == 0:
        return totals, member
    for i in range(n_splits):
        cal, test = roles_eager(seed, r0 + i, unit, within, ucount, cal_thr)
        totals[i] = torch.stack([(cal & ~z).sum(), (cal & z).sum(), (test & ~z).sum(), (test & z).sum()]).to(torch.int32)
        for st in range(strata):
            mask = cal if strata == 1 else (cal & z if st else cal & ~z)
            csum = torch.cumsum(mask.long(), 0)
            n_cal = csum[-1]
            k = rank_k(n_cal, ppm)
            target = n_cal - k + 1 if st else k
            pos = torch.searchsorted(csum, target.clamp(min=1))   # the first window with csum >= target
            member[i, st] = torch.where(k <= n_cal, pos, torch.full_like(pos, -1)).to(torch.int32)
    return totals, member


def count_eager(unit: torch.Tensor, packed: torch.Tensor, within: Optional[torch.Tensor], ucount: Optional[torch.Tensor],
                seed: int, r0: int, cal_thr: int, cuts: torch.Tensor) -> torch.Tensor:
    """``conformal_count_kernel`` in torch (any device), one split at a time."""
    if cuts.dim() != 2 or cuts.dtype != torch.int32 or not 1 <= cuts.shape[1] <= MAX_CUTS:
        raise ValueError(f"cuts must be (R, Q) int32, Q in 1..{MAX_CUTS}")
    n_splits = cuts.shape[0]
    _check_roles(unit, packed, within, ucount, cal_thr, r0, n_splits)
    dev, n = unit.device, unit.numel()
    out = torch.zeros(n_splits, cuts.shape[1], 2, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    z = (packed & Z_BIT) != 0
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    for i in range(n_splits):
        _, test = roles_eager(seed, r0 + i, unit, within, ucount, cal_thr)
        c = cuts[i].long().to(dev).clamp(0, n)
        for cls, m in enumerate((test & ~z, test & z)):
            out[i, :, cls] = torch.cat([zero, torch.cumsum(m.long(), 0)])[c].to(torch.int32)
    return out


def _segments(segments: int) -> int:
    if not 0 <= int(segments) <= MAX_SEGMENTS:
        raise ValueError(f"segments must be in 0..{MAX_SEGMENTS}")
    return int(segments)


def select(unit: torch.Tensor, packed: torch.Tensor, within: Optional[torch.Tensor], ucount: Optional[torch.Tensor],
           seed: int, r0: int, n_splits: int, cal_thr: int, alpha_ppm: torch.Tensor, strata: int,
           segments: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Totals (R, 4) int32 ``cal0, cal1, test0, test1`` and members (R, strata, A) int32 of splits ``r0 .. r0 + R - 1``:
    the HIP kernel on the GPU, else :func:`select_eager`.  Stratum 0 (or the single stratum, which ignores the
    class): the window of rank ``k`` among the calibration windows in ascending order; stratum 1: the k-th
    largest of class 1; ``-1`` where ``k > n_cal``.  ``segments`` caps the segments the kernel cuts a row into
    (0: its maximum); the result does not depend on it."""
    seed = int(seed) & 0xFFFFFFFF
    if unit.is_cuda and unit.numel() > 0 and n_splits > 0:
        return _ext.ops().conformal_select(unit, packed, within, ucount, seed, int(r0), int(n_splits), int(cal_thr),
                                           alpha_ppm.to(device=unit.device, dtype=torch.int32), int(strata),
                                           _segments(segments))
    return select_eager(unit, packed, within, ucount, seed, r0, n_splits, cal_thr, alpha_ppm, strata)


def count(unit: torch.Tensor, packed: torch.Tensor, within: Optional[torch.Tensor], ucount: Optional[torch.Tensor],
          seed: int, r0: int, cal_thr: int, cuts: torch.Tensor, segments: int = 0) -> torch.Tensor:
    """(R, Q, 2) int32: the test windows of class 0 / 1 among sorted positions ``[0, cuts[r, q])`` in split ``r0 + r``."""
    seed = int(seed) & 0xFFFFFFFF
    if unit.is_cuda and unit.numel() > 0 and cuts.shape[0] > 0:
        return _ext.ops().conformal_count(unit, packed, within, ucount, seed, int(r0), int(cal_thr),
                                          cuts.to(device=unit.device, dtype=torch.int32), _segments(segments))
    return count_eager(unit, packed, within, ucount, seed, r0, cal_thr, cuts)


def group_bounds(start: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(group_start, group_end)`` (n,) int64 per sorted window from the tie-group-start flags: the first
    position of its tie group and one past the last (the ``cummax`` trick of ``rank.split_bounds``)."""
    n = start.numel()
    ar = torch.arange(n, dtype=torch.int64, device=start.device)
    if n == 0:
        return ar, ar
    s = start.clone()
    s[0] = True
    gs = torch.cummax(torch.where(s, ar, torch.zeros_like(ar)), 0).values
    nxt = torch.cat([s[1:], torch.ones(1, dtype=torch.bool, device=start.device)])   # the next window starts a group
    ge = n - torch.cummax(torch.where(nxt, n - 1 - ar, torch.zeros_like(ar)).flip(0), 0).values.flip(0)
    return gs, ge


def assemble(totals: torch.Tensor, tz: torch.Tensor, e0: torch.Tensor, s1: torch.Tensor) -> torch.Tensor:
    """(R, A, 10) int64 counts ``COLS`` from the totals (R, 4), the prefix counts ``tz`` (R, 2 A, 2) at the cuts
    ``[e0 | s1]`` and the cuts themselves (R, A)."""
    n_alpha = e0.shape[1]
    t = tz.long()
    te, ts = t[:, :n_alpha], t[:, n_alpha:]                       # (R, A, 2): T_z(e0), T_z(s1)
    n_test = totals.long()[:, 2:4][:, None, :].expand_as(te)
    wide = (e0 >= s1)[..., None]
    zero = torch.zeros_like(te)
    cols = [n_test, te, n_test - ts, torch.where(wide, te - ts, zero), torch.where(wide, zero, ts - te)]
    return torch.cat([torch.stack([c[..., z] for c in cols], dim=-1) for z in (0, 1)], dim=-1)


def finalize(counts) -> Dict[str, np.ndarray]:
    """(..., 10) integer counts ``COLS`` -> float64 ``METRICS`` and the integer ``n_valid`` (the windows counted),
    each of the leading shape.  A ratio without a denominator is NaN."""
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.astype(np.int64)
    if c.shape[-1] != len(COLS):
        raise ValueError(f"counts do not have {len(COLS)} columns")
    g = {name: c[..., i] for i, name in enumerate(COLS)}

    def ratio(num, den):
        ok = den > 0
        return np.where(ok, num.astype(np.float64) / np.where(ok, den, 1).astype(np.float64), np.nan)

    n = g["n_test_0"] + g["n_test_1"]
    both, empty = g["both_0"] + g["both_1"], g["empty_0"] + g["empty_1"]
    single = n - both - empty
    right = (g["incl0_0"] - g["both_0"]) + (g["incl1_1"] - g["both_1"])
    return {
        "coverage": ratio(g["incl0_0"] + g["incl1_1"], n),
        "coverage_class_0": ratio(g["incl0_0"], g["n_test_0"]),
        "coverage_class_1": ratio(g["incl1_1"], g["n_test_1"]),
        "share_empty": ratio(empty, n),
        "share_singleton": ratio(single, n),
        "share_both": ratio(both, n),
        "mean_set_size": ratio(g["incl0_0"] + g["incl0_1"] + g["incl1_0"] + g["incl1_1"], n),
        "singleton_accuracy": ratio(right, single),
        "n_valid": n.copy(),
    }
