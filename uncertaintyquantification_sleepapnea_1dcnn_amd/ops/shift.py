"""Signal corruptions of the shift sweep: the HIP kernel (``csrc/uq_shift.hip``) and its torch float64 emulation,
which is also the CPU path.

A window is ``(L, C)``, time-major (``X[n, t, c]``), fp32 or fp64.  ``mu_c`` / ``sigma_c`` are the mean and population
std of channel c of the *clean* window in fp64; every corruption is stated in units of ``sigma_c`` and so means the
same on raw and on standardised windows.  A condition is ``(kind, p, channel mask)``; severity 1..5 picks ``p`` from
:data:`SEVERITY`, severity 0 (kind ``none``) is "no corruption".  With ``restandardize`` the corrupted window goes
through the pipeline's per-window standardisation ``(x' - mean') / (std' + 1e-8)`` again
(``data/prepare.py:standardize_per_window``), so a dead channel is fed as zeros.

=================  ===========================================================================  =====================
kind               corrupted value ``x'_t``                                                     ``p`` at severity 1..5
=================  ===========================================================================  =====================
``gaussian_noise``  ``x_t + p sigma g_t``                                                        0.1, 0.25, 0.5, 1, 2
``flatline``        ``l = clamp(floor(p L + 0.5), 1, L)``, start ``s = (h (L - l + 1)) >> 32``;   0.1, 0.25, 0.5, 0.75, 1
                    for t in [s, s + l): ``x_{max(s - 1, 0)}`` (a stuck sensor)
``spikes``          where ``u16(t) < rint(p 65536)``: ``mu +/- 6 sigma`` (motion artefacts)       0.02, 0.05, 0.1, 0.2, 0.4
``drift``           ``x_t + sign p sigma t / (L - 1)``, one sign per (window, channel); nothing    0.5, 1, 2, 4, 8
                    at L = 1
``clip``            ``clamp(x_t, mu - p sigma, mu + p sigma)`` (saturation)                       2, 1.5, 1, 0.5, 0.25
``delay``           ``x_{max(t - d, 0)}``, ``d = min(int(p), L - 1)`` (a desynchronised channel)  1, 2, 4, 8, 16
``quantize``        ``mu + q sigma rint((x_t - mu) / (q sigma))``, q = p, ties to even;           0.25, 0.5, 1, 1.5, 2
                    unchanged where ``sigma = 0``
=================  ===========================================================================  =====================

The noise is ``g_t = (S - 131070) / sqrt((65536^2 - 1) / 3)`` with S the sum of the four 16-bit halves of two hash
words: no transcendental function, variance exactly 1 by construction, kurtosis 2.7 (a sum of four uniforms, not a
normal deviate) and ``|g| <= 2 sqrt(3)``.  A gain or offset corruption is absent on purpose: per-window
standardisation removes it.

Randomness is the counter hash of ``ops/rng.py``: the key is ``shift_key(seed, kind, channel, global window index)``
and a draw is ``shift_word(key, counter)``.  The severity is not in the key, so all severities of a kind share their
draws: curves over severity are paired and spike positions are nested.  ``window_offset`` makes a shard's result
the slice of the whole set's.

The moments are ``mean = x_0 + sum(x_t - x_0) / L`` and ``std = sqrt(sum((x_t - mean)^2) / L)`` (a constant channel
gives exactly ``std = 0`` and zeros), each sum taken in the kernel's order: a lane adds its rows ``t = l, l + 64, ...``,
then the 64 lanes are added by halving.  :func:`corrupt_eager` uses the same order and the same operations; the two
are not guaranteed to agree to the bit (measured: bitwise after the rounding to fp32 in most cases, not all), and
the GPU tests hold the kernel to ``|got - ref64| <= 2^-23 |ref64| + 1e-12``.

Kernel limits: C <= 4, L <= 256, K <= 64 per launch, 2^27 windows; outside them (and off the GPU)
:func:`shift_corrupt` runs the emulation, on a GPU tensor with one warning.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional, Sequence, Tuple

import torch

from . import _ext, rng

KINDS = ("none", "gaussian_noise", "flatline", "spikes", "drift", "clip", "delay", "quantize")
NONE, NOISE, FLATLINE, SPIKES, DRIFT, CLIP, DELAY, QUANTIZE = range(8)
SEVERITY = {
    "gaussian_noise": (0.1, 0.25, 0.5, 1.0, 2.0),
    "flatline": (0.1, 0.25, 0.5, 0.75, 1.0),
    "spikes": (0.02, 0.05, 0.1, 0.2, 0.4),
    "drift": (0.5, 1.0, 2.0, 4.0, 8.0),
    "clip": (2.0, 1.5, 1.0, 0.5, 0.25),
    "delay": (1.0, 2.0, 4.0, 8.0, 16.0),
    "quantize": (0.25, 0.5, 1.0, 1.5, 2.0),
}
MAX_C, MAX_L, MAX_K, MAX_N = 4, 256, 64, 1 << 27     # uq_api.h kShiftMax*
EPS = 1e-8
NOISE_MEAN = 131070.0
NOISE_SCALE = 37837.22723720648                        # sqrt((65536^2 - 1) / 3), uq_shift.hip kNoiseScale
LANES = 64

_warned = set()


# ===================== Conditions =====================
def kind_code(kind) -> int:
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}")
        return KINDS.index(kind)
    if not 0 <= int(kind) < len(KINDS):
        raise ValueError(f"kind code must be in 0..{len(KINDS) - 1}")
    return int(kind)


def severity_param(kind, severity: int) -> float:
    """``p`` of a kind at severity 1..5 (0.0 at severity 0)."""
    code = kind_code(kind)
    if int(severity) != severity or not 0 <= severity <= 5:
        raise ValueError("severity must be an integer in 0..5")
    return 0.0 if severity == 0 or code == NONE else float(SEVERITY[KINDS[code]][int(severity) - 1])


def channel_mask(channels: Optional[Sequence[int]], C: int) -> int:
    """Bit c set: the kind applies to channel c.  ``None`` is every channel."""
    if channels is None:
        return (1 << C) - 1
    m = 0
    for c in channels:
        if not 0 <= int(c) < C:
            raise ValueError(f"channel {c} is not in 0..{C - 1}")
        m |= 1 << int(c)
    return m


def condition(kind, severity: Optional[int] = None, p: Optional[float] = None,
              channels: Optional[Sequence[int]] = None, C: int = MAX_C) -> Tuple[int, float, int]:
    """``(kind code, p, channel mask)`` from a severity 0..5 or a float ``p`` given directly."""
    code = kind_code(kind)
    if (severity is None) == (p is None):
        raise ValueError("give either severity or p")
    if p is None:
        if severity == 0:
            code = NONE
        p = severity_param(code, severity)
    p = float(p)
    if not (math.isfinite(p) and p >= 0.0):
        raise ValueError("p must be finite and non-negative")
    return code, p, channel_mask(channels, C)


def supports(n: int, L: int, C: int, K: int) -> bool:
    return 1 <= C <= MAX_C and 1 <= L <= MAX_L and 1 <= K <= MAX_K and n <= MAX_N


# ===================== The emulation =====================
def _wave_sum(a: torch.Tensor) -> torch.Tensor:
    """Sum over dim 1 (time) of (n, L, C) in the kernel's order; returns (n, 1, C)."""
    n, L, C = a.shape
    R = -(-L // LANES)
    if R * LANES != L:
        a = torch.cat([a, a.new_zeros(n, R * LANES - L, C)], dim=1)
    a = a.reshape(n, R, LANES, C)
    acc = a.new_zeros(n, LANES, C)
    for j in range(R):
        acc = acc + a[:, j]
    h = LANES // 2
    while h >= 1:
        acc = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    return acc


def moments(v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mean, std)`` (n, 1, C) over time of (n, L, C) float64, relative to the first step."""
    L = v.shape[1]
    pivot = v[:, :1]
    mean = pivot + _wave_sum(v - pivot) / float(L)
    d = v - mean
    return mean, torch.sqrt(_wave_sum(d * d) / float(L))


def noise_draws(seed: int, window: torch.Tensor, L: int, C: int) -> torch.Tensor:
    """The unit-variance draws ``g`` (n, L, C) float64 of ``gaussian_noise`` for global window indices ``window``."""
    dev = window.device
    key = rng.shift_key(seed, NOISE, torch.arange(C, device=dev)[None, None, :], window.to(torch.int64)[:, None, None])
    t4 = torch.arange(L, device=dev, dtype=torch.int64)[None, :, None] << 2
    h0, h1 = rng.shift_word(key, t4), rng.shift_word(key, t4 | 1)
    s = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16)
    return (s.double() - NOISE_MEAN) / NOISE_SCALE


def spike_draws(seed: int, window: torch.Tensor, L: int, C: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(u16, positive)`` (n, L, C) of ``spikes``: a step spikes where ``u16 < rint(p 65536)``."""
    dev = window.device
    key = rng.shift_key(seed, SPIKES, torch.arange(C, device=dev)[None, None, :], window.to(torch.int64)[:, None, None])
    h = rng.shift_word(key, torch.arange(L, device=dev, dtype=torch.int64)[None, :, None] << 2)
    return h & 0xFFFF, ((h >> 16) & 1) == 1


def flatline_run(seed: int, window: torch.Tensor, L: int, C: int, p: float) -> Tuple[torch.Tensor, int]:
    """``(start (n, 1, C), length)`` of the held run of ``flatline``."""
    dev = window.device
    length = int(min(max(math.floor(p * L + 0.5), 1.0), float(L)))
    key = rng.shift_key(seed, FLATLINE, torch.arange(C, device=dev)[None, None, :], window.to(torch.int64)[:, None, None])
    return (rng.shift_word(key, rng.SHIFT_WINDOW_CTR) * (L - length + 1)) >> 32, length


def _corrupt_one(x: torch.Tensor, mu: torch.Tensor, sg: torch.Tensor, code: int, p: float, seed: int,
                 window: torch.Tensor) -> torch.Tensor:
    n, L, C = x.shape
    dev = x.device
    t = torch.arange(L, device=dev, dtype=torch.int64)[None, :, None]
    if code == NOISE:
        return x + (p * sg) * noise_draws(seed, window, L, C)
    if code == FLATLINE:
        start, length = flatline_run(seed, window, L, C, p)
        hold = torch.gather(x, 1, (start - 1).clamp(min=0))
        return torch.where((t >= start) & (t < start + length), hold, x)
    if code == SPIKES:
        thr = int(min(max(round(p * 65536.0), 0), 65536))   # Python rounds half to even, like rint
        u16, pos = spike_draws(seed, window, L, C)
        a = 6.0 * sg
        return torch.where(u16 < thr, torch.where(pos, mu + a, mu - a), x)
    if code == DRIFT:
        if L == 1:
            return x.clone()
        key = rng.shift_key(seed, DRIFT, torch.arange(C, device=dev)[None, None, :], window[:, None, None])
        a = torch.where((rng.shift_word(key, rng.SHIFT_WINDOW_CTR) & 1) == 1, p * sg, -(p * sg))
        return x + (a * t.double()) / float(L - 1)
    if code == CLIP:
        a = p * sg
        return torch.minimum(torch.maximum(x, mu - a), mu + a)
    if code == DELAY:
        d = int(min(p, float(L - 1)))
        return torch.gather(x, 1, (t - d).clamp(min=0).expand(n, L, C))
    if code == QUANTIZE:
        a = p * sg
        safe = torch.where(a > 0.0, a, torch.ones_like(a))
        return torch.where(a > 0.0, mu + a * torch.round((x - mu) / safe), x)
    return x.clone()


def _cond_lists(kinds, params, chmask):
    kk = [int(v) for v in torch.as_tensor(kinds).reshape(-1).tolist()]
    pp = [float(v) for v in torch.as_tensor(params, dtype=torch.float64).reshape(-1).tolist()]
    mm = [int(v) for v in torch.as_tensor(chmask).reshape(-1).tolist()]
    if not (len(kk) == len(pp) == len(mm)) or not kk:
        raise ValueError("kinds, params and chmask must hold the same number (>= 1) of conditions")
    for k, p in zip(kk, pp):
        kind_code(k)
        if not (math.isfinite(p) and p >= 0.0):
            raise ValueError("p must be finite and non-negative")
    return kk, pp, mm


def _check_x(x: torch.Tensor, window_offset: int) -> None:
    if x.dim() != 3 or x.dtype not in (torch.float32, torch.float64) or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("x must be (n, L, C) float32 or float64")
    if window_offset < 0 or window_offset + x.shape[0] > (1 << 32):
        raise ValueError("window_offset + n must stay within 2^32")


def corrupt_eager(x: torch.Tensor, kinds, params, chmask, seed: int, window_offset: int = 0,
                  restandardize: bool = True) -> torch.Tensor:
    """(K, n, L, C) float64 on ``x``'s device: condition k = ``(kinds[k], params[k], chmask[k])`` of every window,
    in torch float64 with the kernel's operations in the kernel's order."""
    _check_x(x, window_offset)
    kk, pp, mm = _cond_lists(kinds, params, chmask)
    n, L, C = x.shape
    x64 = x.double()
    window = torch.arange(n, device=x.device, dtype=torch.int64) + int(window_offset)
    mu, sg = moments(x64)
    cbit = 1 << torch.arange(C, device=x.device, dtype=torch.int64)
    out = []
    for code, p, m in zip(kk, pp, mm):
        if m < 0 or m >= (1 << C):
            raise ValueError("chmask must hold bits of channels 0..C-1")
        y = _corrupt_one(x64, mu, sg, code, p, seed, window)
        y = torch.where(((cbit & m) != 0)[None, None, :], y, x64)
        if restandardize:
            m2, s2 = moments(y)
            y = (y - m2) / (s2 + EPS)
        out.append(y)
    return torch.stack(out)


# ===================== Dispatch =====================
def warn_unsupported(shape, K: int) -> None:
    """One warning per shape: the HIP kernel holds C <= 4, L <= 256, K <= 64, 2^27 windows."""
    key = (shape[1], shape[2], K > MAX_K, shape[0] > MAX_N)
    if key not in _warned:
        _warned.add(key)
        warnings.warn(f"shift_corrupt: no HIP kernel for windows {tuple(shape)} with K = {K} (limits C <= {MAX_C}, "
                      f"L <= {MAX_L}, K <= {MAX_K}, 2^27 windows); running the torch float64 formulation",
                      RuntimeWarning, stacklevel=3)


def shift_corrupt(x: torch.Tensor, kinds, params, chmask, seed: int, window_offset: int = 0,
                  restandardize: bool = True) -> torch.Tensor:
    """(K, n, L, C) float32 on ``x``'s device: the HIP kernel on the GPU, else :func:`corrupt_eager` rounded once."""
    _check_x(x, window_offset)
    kk, pp, mm = _cond_lists(kinds, params, chmask)
    n, L, C = x.shape
    if x.is_cuda and supports(n, L, C, len(kk)):
        return _ext.ops().shift_corrupt(x, torch.tensor(kk, dtype=torch.int64), torch.tensor(pp, dtype=torch.float64),
                                        torch.tensor(mm, dtype=torch.int64), int(seed), int(window_offset),
                                        bool(restandardize))
    if x.is_cuda:
        warn_unsupported(x.shape, len(kk))
    return corrupt_eager(x, kk, pp, mm, seed, window_offset, restandardize).float()
