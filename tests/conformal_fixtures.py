"""Probabilities, labels, units and the comparison against the golden shared by the conformal-prediction tests."""
import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import conformal as ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import conformal as CF

from .rank_fixtures import STRUCTURES as RANK_STRUCTURES
from .rank_fixtures import make_scores

# the score structures of the rank tests, plus probabilities saturated at 0 / 1 and probabilities below 2^-29
# (distinct in fp32, one tie group after 1 - p in float64)
STRUCTURES = RANK_STRUCTURES + ("saturated", "tiny")
UNITS = ("windows", "few", "one")
ALPHAS = (0.01, 0.05, 0.1, 0.2, 0.5)
SEED = 77
TOL = 1e-12   # float64 metrics: the same integers, one division each


def make_case(n, structure, seed=3):
    """fp32 probabilities correlated with the labels, and the labels (about 30 % positives)."""
    if structure in RANK_STRUCTURES:
        s, y = make_scores(n, structure, seed)
        return (s if structure == "equal" else (s / np.float32(1.35)).astype(np.float32)), y
    rs = np.random.RandomState(seed + n)
    y = (rs.rand(n) > 0.7).astype(np.int32)
    if structure == "saturated":
        p = (rs.rand(n) + 0.35 * y > 0.7).astype(np.float32)
        mid = rs.rand(n) < 0.1
        p[mid] = rs.rand(int(mid.sum())).astype(np.float32)
        return p, y
    return (rs.rand(n) * 2.0 ** -30 * (1 + y)).astype(np.float32), y


def make_ids(n, units, seed=5):
    """Patient ids per window (None: every window is its own unit)."""
    if units == "windows":
        return None
    if units == "one":
        return np.full(n, 42, np.int64)
    rs = np.random.RandomState(seed + n)
    return rs.randint(0, max(2, min(12, n)), size=n).astype(np.int64) * 3 + 100


def prepare(p, y, ids, cluster, mode, device="cpu"):
    return CF._prepare(torch.as_tensor(p).to(device), y, ids, cluster, mode)


def check_against_golden(p, y, ids, cluster, mode, cal_fraction=0.5, n_splits=3, alphas=ALPHAS, r0=0, seed=SEED):
    """Emulation (select_eager / count_eager / assemble / finalize on the CPU) against the literal golden of every
    split and level: integer counts equal, metrics within TOL, totals equal to the sizes of the role masks."""
    ppm = ops.alpha_to_ppm(alphas)
    pp = prepare(p, y, ids, cluster, mode)
    totals, counts = CF._split_counts(pp, seed, r0, n_splits, ops.cal_threshold(cal_fraction),
                                      torch.as_tensor(ppm, dtype=torch.int32), mode)
    assert totals.dtype == torch.int32 and tuple(counts.shape) == (n_splits, len(ppm), 10)
    fin = ops.finalize(counts)
    yy = np.asarray(y)
    for i in range(n_splits):
        cal, test = CF.split_masks(p, seed, r0 + i, cal_fraction, ids, cluster)
        want = [int((cal & (yy == 0)).sum()), int((cal & (yy == 1)).sum()), int((test & (yy == 0)).sum()),
                int((test & (yy == 1)).sum())]
        assert totals[i].tolist() == want
        for j, a in enumerate(ppm):
            g = CF.golden_conformal_split(p, y, cal, test, int(a), mode)
            got = dict(zip(ops.COLS, counts[i, j].tolist()))
            assert got == g["counts"], (i, int(a), got, g["counts"])
            for m in ops.METRICS:
                x, ref = float(fin[m][i, j]), g[m]
                assert (np.isnan(x) and np.isnan(ref)) or abs(x - ref) <= TOL, (m, x, ref)
            assert int(fin["n_valid"][i, j]) == g["n_valid"]
    return totals, counts
