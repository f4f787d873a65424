"""Calibration / selective prediction on the CPU: the float64 golden functions against hand-computed
values, and the integer emulation of the HIP kernels (``ops/calib.py``) against the golden."""
import os

import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import calib
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M

# One quantum of p_q / brier_q, and of nll_q: per window the quantised value is within half a quantum
# of the exact one, so is every mean of them.
TOL_P = 1.0 / calib.P_SCALE
TOL_NLL = 1.0 / calib.NLL_SCALE
COUNT_KEYS = ("bin_count", "coverage", "accuracy", "sensitivity", "specificity")
N, T, K, B = 2000, 7, 15, 20
COVERAGES = np.linspace(0.5, 1.0, 11)


def test_golden_hand_checked():
    p = np.array([0.1, 0.4, 0.6, 0.9, 0.9, 0.2])
    y = np.array([0, 1, 1, 1, 0, 0])
    g = C.golden_calibration(p, y, n_bins=5)
    # bins of width 0.2: {0.1} -> 0, {0.2} -> 1 (0.2 * 5 = 1.0), {0.4} -> 2, {0.6} -> 3, {0.9, 0.9} -> 4
    assert g["bin_count"].tolist() == [1, 1, 1, 1, 2]
    gaps = [abs(0 - 0.1), abs(0 - 0.2), abs(1 - 0.4), abs(1 - 0.6), abs(0.5 - 0.9)]
    ece = (gaps[0] + gaps[1] + gaps[2] + gaps[3] + 2 * gaps[4]) / 6
    brier = (0.1 ** 2 + 0.6 ** 2 + 0.4 ** 2 + 0.1 ** 2 + 0.9 ** 2 + 0.2 ** 2) / 6
    nll = -(np.log(0.9) + np.log(0.4) + np.log(0.6) + np.log(0.9) + np.log(0.1) + np.log(0.8)) / 6
    assert abs(g["ece"] - ece) < 1e-12
    assert abs(g["mce"] - 0.6) < 1e-12
    assert abs(g["brier"] - brier) < 1e-12
    assert abs(g["nll"] - nll) < 1e-12
    np.testing.assert_allclose(g["bin_confidence"], [0.1, 0.2, 0.4, 0.6, 0.9], atol=1e-12)
    np.testing.assert_allclose(g["bin_frequency"], [0, 0, 1, 1, 0.5], atol=1e-12)
    # refer the two most uncertain windows (score = closeness to 0.5): 0.4 (wrong) and 0.6 (right)
    s = -np.abs(p - 0.5)
    sel = C.golden_selective(p, s, y, [np.sort(s)[3], np.sort(s)[5]])
    np.testing.assert_allclose(sel["coverage"], [4 / 6, 1.0], atol=1e-12)
    np.testing.assert_allclose(sel["accuracy"], [3 / 4, 4 / 6], atol=1e-12)  # 0.9 with y = 0 and 0.4 with y = 1 are wrong
    np.testing.assert_allclose(sel["sensitivity"], [1.0, 2 / 3], atol=1e-12)
    np.testing.assert_allclose(sel["specificity"], [2 / 3, 2 / 3], atol=1e-12)
    assert abs(sel["aurc"] - 0.5 * (1 / 4 + 1 / 3) * (1 - 4 / 6)) < 1e-12


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(1)
    probs = rs.rand(T, N).astype(np.float32)
    y = (rs.rand(N) > 0.7).astype(np.int32)
    p, s = C.per_window(probs, "total_pred_entropy")
    thr = C.coverage_thresholds(s, COVERAGES)
    rec = calib.prep_eager(p, s, torch.from_numpy(y), torch.from_numpy(thr), K)
    return {"probs": probs, "y": y, "p": p, "s": s, "thr": thr, "rec": rec,
            "p64": p.numpy().astype(np.float64), "s_np": s.numpy()}


def _compare(got, ref):
    # every retained set and both classes are non-empty, so nothing here may hide behind the NaN rule; the
    # only NaNs are the confidence / frequency of the empty bins (the mean of 7 uniforms leaves the outer
    # bins empty), and they must sit exactly on the bins whose count is 0
    for k in ("bin_count", "coverage", "accuracy", "sensitivity", "specificity", "ece", "mce", "brier", "nll", "aurc"):
        assert not np.isnan(np.asarray(ref[k], dtype=np.float64)).any(), k
        assert not np.isnan(np.asarray(got[k], dtype=np.float64)).any(), k
    empty = np.asarray(ref["bin_count"]) == 0
    assert not empty.all()
    for k in ("bin_confidence", "bin_frequency"):
        np.testing.assert_array_equal(np.isnan(got[k]), empty, err_msg=k)
        np.testing.assert_array_equal(np.isnan(ref[k]), empty, err_msg=k)
    for k in COUNT_KEYS + ("bin_frequency",):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    d = np.abs(got["bin_confidence"] - ref["bin_confidence"])[~empty]
    assert d.max() <= TOL_P, ("bin_confidence", d.max())
    for k in ("ece", "mce", "brier"):
        assert np.max(np.abs(got[k] - ref[k])) <= TOL_P, (k, np.max(np.abs(got[k] - ref[k])))
    assert np.max(np.abs(got["nll"] - ref["nll"])) <= TOL_NLL
    # a sum of 10 trapezoids of exactly equal count ratios: only fp64 rounding of the two summation orders
    assert np.max(np.abs(got["aurc"] - ref["aurc"])) <= 1e-12


@pytest.mark.parametrize("parity", [True, False])
def test_emulation_matches_golden(data, parity):
    if parity:
        idx = M.parity_bootstrap_indices(N, B, 2025)
        sums = calib.bootstrap_sums(data["rec"], B, K, len(data["thr"]), idx=torch.from_numpy(idx))
    else:
        idx = uq_ops._hash_idx(N, B, 2025, "cpu").numpy()
        sums = calib.bootstrap_sums(data["rec"], B, K, len(data["thr"]), seed=2025)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (B, calib.n_columns(K, len(data["thr"])))
    got = calib.finalize(sums, N, K, len(data["thr"]))
    ref = C.golden_replicates(data["p64"], data["s_np"], data["y"], data["thr"], idx, K)
    _compare(got, ref)
    # point estimates: the same path with idx = arange(n)
    pt = calib.finalize(calib.bootstrap_sums(data["rec"], 1, K, len(data["thr"]), idx=torch.arange(N)[None])[0], N, K,
                        len(data["thr"]))
    ref_pt = {**C.golden_calibration(data["p64"], data["y"], K),
              **C.golden_selective(data["p64"], data["s_np"], data["y"], data["thr"])}
    _compare(pt, ref_pt)
    assert pt["coverage"][-1] == 1.0 and np.all(pt["coverage"] >= COVERAGES - 1e-12)


def test_public_point_functions(data):
    cm = C.calibration_metrics(data["probs"], data["y"], n_bins=K)
    ref = C.golden_calibration(data["p64"], data["y"], K)
    np.testing.assert_array_equal(cm["bin_count"], ref["bin_count"])
    assert abs(cm["ece"] - ref["ece"]) <= TOL_P and abs(cm["nll"] - ref["nll"]) <= TOL_NLL
    sp = C.selective_prediction(data["probs"][:, :, None], data["y"], score="mutual_info", coverages=[0.8, 1.0])
    s = uq_ops.metrics(torch.from_numpy(data["probs"]))[uq_ops.MI].numpy()
    assert sp["thresholds"][0] == np.sort(s)[int(np.ceil(0.8 * N)) - 1] and sp["thresholds"][1] == s.max()
    ref = C.golden_selective(data["p64"], s, data["y"], sp["thresholds"])
    for k in ("coverage", "accuracy", "sensitivity", "specificity"):
        np.testing.assert_array_equal(sp[k], ref[k])
    # an explicit (N,) score and (N,) predictions
    sp1 = C.selective_prediction(data["p"].numpy(), data["y"], score=s, coverages=[0.8, 1.0])
    np.testing.assert_array_equal(sp1["accuracy"], sp["accuracy"])


def test_nan_rule(data):
    y0 = np.zeros(N, dtype=np.int32)
    res = C.evaluate_calibration(data["probs"], y0, "allneg", n_bootstrap=5, random_state=3, make_plots=False)
    for sfx in C.coverage_suffixes(COVERAGES):
        for end in ("", "_mean", "_ci_lower", "_ci_upper"):
            assert np.isnan(res[f"sensitivity{sfx}{end}"])
            assert not np.isnan(res[f"specificity{sfx}{end}"])
    assert not np.isnan(res["aurc"]) and not np.isnan(res["ece_ci_upper"])


def test_shard_additivity(data):
    n = 3001
    rs = np.random.RandomState(5)
    p = torch.from_numpy(rs.rand(n).astype(np.float32))
    s = torch.from_numpy(rs.rand(n).astype(np.float32))
    y = torch.from_numpy((rs.rand(n) > 0.6).astype(np.int32))
    thr = torch.from_numpy(C.coverage_thresholds(s, COVERAGES))
    rec = calib.prep_eager(p, s, y, thr, K)
    J = thr.numel()
    for idx in (torch.from_numpy(M.parity_bootstrap_indices(n, 6, 7)), None):
        full = calib.bootstrap_sums(rec, 6, K, J, idx=idx, seed=7)
        assert torch.equal(full[:, 0:3 * K:3].sum(1), torch.full((6,), n))
        tot = torch.zeros_like(full)
        for lo, hi in ((0, 1000), (1000, 1001), (1001, 3001)):
            tot += calib.bootstrap_sums(rec[lo:hi], 6, K, J, idx=idx, seed=7, n_global=n, lo=lo)
        assert torch.equal(tot, full)
        # the launch grid is not part of the result (on the CPU the argument is accepted and ignored)
        assert torch.equal(calib.bootstrap_sums(rec, 6, K, J, idx=idx, seed=7, slices=1),
                           calib.bootstrap_sums(rec, 6, K, J, idx=idx, seed=7, slices=3))


def test_hash_row_matches_bootstrap_hash():
    full = uq_ops._hash_idx(777, 5, 2025, "cpu")
    for b in range(5):
        assert torch.equal(calib._hash_row(777, b, 2025, "cpu"), full[b])


def test_evaluate_calibration(data, tmp_path):
    out = str(tmp_path / "plots")
    res = C.evaluate_calibration(data["probs"], data["y"], "unit", n_bootstrap=B, random_state=2025,
                                 output_plot_dir=out)
    suf = C.coverage_suffixes(COVERAGES)
    assert suf[0] == "_at_0.50" and suf[6] == "_at_0.80" and suf[-1] == "_at_1.00"
    with_ci = list(C.CI_SCALARS) + [f"{k}{s}" for s in suf for k in C.CI_CURVES]
    keys = set(with_ci) | {f"coverage{s}" for s in suf}
    keys |= {f"{k}{e}" for k in with_ci for e in ("_mean", "_ci_lower", "_ci_upper")}
    assert set(res) == keys
    assert all(isinstance(v, float) for v in res.values())
    for k in with_ci:
        assert res[f"{k}_ci_lower"] <= res[f"{k}_mean"] <= res[f"{k}_ci_upper"], k
    acc = float(np.mean((data["p64"] > 0.5) == (data["y"] == 1)))
    assert res["accuracy_at_1.00"] == acc and res["coverage_at_1.00"] == 1.0
    # hash resampling: another stream, same point values
    res_h = C.evaluate_calibration(data["probs"], data["y"], "unit", n_bootstrap=B, random_state=2025, parity=False,
                                   make_plots=False)
    assert res_h["ece"] == res["ece"] and res_h["ece_mean"] != res["ece_mean"]
    if C.plt is not None:
        assert os.path.exists(os.path.join(out, "reliability_unit.png"))
        assert os.path.exists(os.path.join(out, "accuracy_coverage_unit.png"))


def test_limits():
    p = torch.rand(10)
    with pytest.raises(ValueError):
        calib.prep(p, p, torch.zeros(10, dtype=torch.int32), torch.zeros(0), 33)
    with pytest.raises(ValueError):
        calib.prep(p, p, torch.zeros(10, dtype=torch.int32), torch.zeros(65), 15)
    with pytest.raises(ValueError):
        C.selective_prediction(p.numpy(), np.zeros(10), score="entropy_bits")


def test_cli(tmp_path):
    import pandas as pd

    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import commands

    rs = np.random.RandomState(0)
    n = 200
    p = rs.rand(n).astype(np.float32)
    df = pd.DataFrame({"Patient_ID": np.nan, "Window_Index": np.arange(n), "True_Label": (rs.rand(n) < p).astype(int),
                       "Predicted_Label": (p > 0.5).astype(int), "Predicted_Probability": p,
                       "Predictive_Variance": rs.rand(n).astype(np.float32) * 0.1,
                       "Predictive_Entropy": M.binary_entropy_bits(p)})
    src, dst = str(tmp_path / "detail.csv"), str(tmp_path / "out" / "calib.csv")
    df.to_csv(src, index=False)
    assert "analyze_calibration" in commands.COMMANDS
    commands.main(["analyze_calibration", "--input_csv", src, "--score", "Predictive_Variance", "--n_bins", "10",
                   "--n_bootstrap", "8", "--seed", "1", "--output_csv", dst, "--no_plots"])
    t = pd.read_csv(dst)
    assert list(t.columns) == ["metric", "value", "mean", "ci_lower", "ci_upper"]
    assert {"ece", "mce", "brier", "nll", "aurc", "accuracy_at_0.80", "coverage_at_1.00"} <= set(t["metric"])
    row = t.set_index("metric").loc["ece"]
    assert row["ci_lower"] <= row["mean"] <= row["ci_upper"]
    assert np.isnan(t.set_index("metric").loc["coverage_at_1.00", "mean"])
