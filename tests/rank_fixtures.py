"""Scores, labels and the comparison against the golden shared by the rank-statistics tests."""
import numpy as np

TOL_RANK = 1e-12   # auroc, u_statistic: integer sums, one rounding
TOL_PR = 1e-9      # pr_auc, average_precision: quantisation n 2^-57 plus fp64 summation n 2^-53, both < 1e-12 here
STRUCTURES = ("continuous", "levels8", "equal")


def make_scores(n, structure, seed=3):
    """fp32 scores correlated with the labels, and the labels (about 30 % positives)."""
    rs = np.random.RandomState(seed + n)
    y = (rs.rand(n) > 0.7).astype(np.int32)
    s = (rs.rand(n) + 0.35 * y).astype(np.float32)
    if structure == "levels8":
        s = (np.floor(s * 8 / 1.35) / 8).astype(np.float32)
    elif structure == "equal":
        s = np.full(n, 0.25, np.float32)
    return s, y


def check_against_golden(fin, gold, b_slice=slice(None)):
    for k, tol in (("auroc", TOL_RANK), ("u_statistic", TOL_RANK), ("pr_auc", TOL_PR), ("average_precision", TOL_PR)):
        got, ref = np.asarray(fin[k])[b_slice], np.asarray(gold[k])[b_slice]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), k
        ok = ~np.isnan(ref)
        err = float(np.max(np.abs(got[ok] - ref[ok]))) if ok.any() else 0.0
        print(f"{k}: max error {err:.3e} (bound {tol:g})")
        assert err <= tol, k
