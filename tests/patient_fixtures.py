"""Deterministic synthetic cohort with a patient-level effect, shared by test_patient_cpu.py and
test_patient_gpu.py: patients differ in prevalence and in how much their passes disagree."""
import numpy as np

TOL_Q = 2.0 ** -30  # one quantum of the fixed-point sums


def cohort(seed, n_pat=40, t_count=20):
    """(probs (T, N) fp32, y (N,) int32, ids (N,) int64), windows grouped by patient, about 4,000 windows."""
    rs = np.random.RandomState(seed)
    n_win = rs.randint(50, 151, size=n_pat)
    prevalence = rs.beta(0.7, 1.5, size=n_pat)
    spread = rs.uniform(0.3, 3.0, size=n_pat)
    ids = np.repeat(np.arange(n_pat), n_win)
    n = ids.size
    y = (rs.rand(n) < prevalence[ids]).astype(np.int32)
    centre = np.where(y == 1, 1.5, -1.5) + rs.randn(n)               # per window
    logit = centre[None, :] + spread[ids][None, :] * rs.randn(t_count, n)   # per pass
    x = logit.astype(np.float32)
    probs = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
    return probs, y, ids


def assert_labels_unambiguous(probs):
    """Precondition of every comparison with the float64 golden: no window's mean is so close to 0.5 that
    the fp32 and the float64 mean could fall on different sides."""
    gap = np.min(np.abs(probs.astype(np.float64).mean(axis=0) - 0.5))
    assert gap > 1e-5, gap


# tolerances of tests/test_kernels_gpu.py::test_uq_reduce_matches_numpy per metric row, plus one quantum
AGG_TOL = {
    "overall_mean_variance": (1e-4, 1e-7 + TOL_Q),
    "mean_variance_class_0": (1e-4, 1e-7 + TOL_Q),
    "mean_variance_class_1": (1e-4, 1e-7 + TOL_Q),
    "mean_total_pred_entropy": (1e-4, 2e-6 + TOL_Q),
    "mean_expected_aleatoric_entropy": (1e-4, 2e-6 + TOL_Q),
    "mean_mutual_info": (1e-3, 5e-6 + TOL_Q),
}
EXACT_COLUMNS = ("num_windows", "num_passes", "hours", "true_index", "true_severity", "pred_index", "pred_severity",
                 "index_mean", "index_std", "index_ci_lower", "index_ci_upper", "p_normal", "p_mild", "p_moderate",
                 "p_severe", "severity_entropy", "severity_confident", "patient_accuracy", "sensitivity", "specificity")
# cohort metrics that are ratios of the same integers in both implementations: only float64 rounding of
# two formulas apart
COUNT_METRICS = ("severity_accuracy", "severity_within_one", "severity_kappa_linear", "ci_coverage", "share_confident",
                 "severity_accuracy_confident", "accuracy", "sensitivity", "specificity")


def check_table(got, ref):
    """Integer-derived columns exact; the two fixed-point means within the uq_reduce tolerances + 2^-30."""
    import numpy.testing as npt

    assert list(got["Patient_ID"]) == list(ref["Patient_ID"])
    for c in EXACT_COLUMNS:
        npt.assert_array_equal(got[c].to_numpy(), ref[c].to_numpy(), err_msg=c)
    npt.assert_allclose(got["mean_variance"], ref["mean_variance"], rtol=1e-4, atol=1e-7 + TOL_Q)
    npt.assert_allclose(got["mean_entropy"], ref["mean_entropy"], rtol=1e-4, atol=2e-6 + TOL_Q)


def check_cohort(got, ref, table, suffix=""):
    """Cohort metrics (or their interval ends, ``suffix``) against the golden.

    Index metrics: a patient's error fraction is quantised to 2^-30, so MAE and bias are within
    60 * 2^-31 events / h.  Limits of agreement: the variance of the error fraction is off by at most
    3 * 2^-31 (mean square and twice bias times mean), so sd by that over 2 sd; with sd > 0.01 asserted
    below, 1.96 * 60 * 3 * 2^-31 / 0.02 = 8.2e-6 events / h.  Pearson r: accuracy and mean entropy are
    quantised to 2^-20 (half a quantum each); with both standard deviations > 0.02 the relative error of
    each centred factor is below 2^-21 / 0.02 = 2.4e-5, four such factors: 1e-4."""
    e = (table["pred_index"] - table["true_index"]).to_numpy() / 60.0
    assert np.std(e) > 0.01 and np.std(table["patient_accuracy"]) > 0.02 and np.std(table["mean_entropy"]) > 0.02
    for k in ("index_mae", "index_bias"):
        assert abs(got[k + suffix] - ref[k]) <= 60 * 2.0 ** -31 + 1e-12, k
    for k in ("index_loa_lower", "index_loa_upper"):
        assert abs(got[k + suffix] - ref[k]) <= 8.2e-6 + 60 * 2.0 ** -31, k
    for k in COUNT_METRICS:
        assert abs(got[k + suffix] - ref[k]) <= 1e-12, k
    assert abs(got["pearson_r_accuracy_entropy" + suffix] - ref["pearson_r_accuracy_entropy"]) <= 1e-4
    for k, (rtol, atol) in AGG_TOL.items():
        assert abs(got[k + suffix] - ref[k]) <= atol + rtol * abs(ref[k]), k
