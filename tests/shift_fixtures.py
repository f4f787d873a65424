"""Inputs and conditions shared by the shift-corruption tests (CPU emulation and GPU kernel)."""
import numpy as np

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import shift as S

SEED = 2025
KIND_CODES = tuple(range(1, len(S.KINDS)))


def windows(n=257, L=60, C=4, seed=7):
    """Raw-looking windows: a scale of up to 50 per channel and an offset of about 10 per (window, channel)."""
    rs = np.random.RandomState(seed)
    return rs.randn(n, L, C) * rs.rand(1, 1, C) * 50 + rs.randn(n, 1, C) * 10


def conditions(C, severities=(1, 5)):
    """Every kind at the severities, on all channels and on the last channel alone: (kinds, params, masks)."""
    kinds, params, masks = [], [], []
    for code in KIND_CODES:
        for sev in severities:
            for m in ((1 << C) - 1, 1 << (C - 1)):
                kinds.append(code)
                params.append(S.severity_param(code, sev))
                masks.append(m)
    return kinds, params, masks


def rint_margin(x64, q):
    """Distance of the arguments of rint in ``quantize`` at step q sigma from the nearest half-integer (min over x)."""
    import torch

    mu, sg = S.moments(x64)
    arg = (x64 - mu) / (q * sg)
    return float((torch.abs(arg - torch.floor(arg) - 0.5)).min())
