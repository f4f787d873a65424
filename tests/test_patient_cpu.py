"""Patient-level severity and the patient-cluster bootstrap on the CPU: a hand-checked example, the eager
integer path (``ops/patient.py``) against the float64 golden of ``uq/patient_level.py``, against the
existing per-patient aggregation, and the cluster interval against the window interval."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.analysis.patient import aggregate_patient_uq_metrics
from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import commands
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import patient as P
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import patient_level as PL
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq.drivers import per_window_table
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq.uq_techniques import bootstrap_metrics, compute_confidence_intervals

from .patient_fixtures import check_cohort, check_table, cohort, assert_labels_unambiguous


@pytest.fixture(autouse=True)
def eager_path(monkeypatch):
    """This file checks the eager emulation, also on a machine with a GPU (test_patient_gpu.py has the kernels)."""
    monkeypatch.setattr(C, "_gpu_ok", lambda: False)


@pytest.fixture(scope="module")
def seed2():
    probs, y, ids = cohort(2)
    assert_labels_unambiguous(probs)
    return probs, y, ids


# 2 patients, 3 and 2 windows, T = 3, 60 s windows: one positive window is 60 / n events per hour
HAND_P = np.array([[0.9, 0.2, 0.7, 0.1, 0.2],
                   [0.8, 0.6, 0.4, 0.3, 0.6],
                   [0.6, 0.1, 0.3, 0.2, 0.1]], dtype=np.float32)
HAND_Y = np.array([1, 0, 1, 0, 0])
HAND_IDS = np.array(["a", "a", "a", "b", "b"])


def test_hand_checked_example():
    pass_pos, rec = P.reduce_eager(torch.from_numpy(HAND_P), uq_ops.metrics_eager(torch.from_numpy(HAND_P)),
                                   torch.from_numpy(HAND_Y), torch.tensor([0, 0, 0, 1, 1], dtype=torch.int32), 2)
    assert pass_pos.tolist() == [[2, 0], [2, 1], [1, 0]]
    # window means 0.767, 0.3, 0.467 | 0.2, 0.3: one predicted positive, a true positive
    assert rec[:, :5].tolist() == [[3, 2, 1, 1, 2], [2, 0, 0, 0, 2]]
    for tbl in (PL.patient_table(HAND_P, HAND_Y, HAND_IDS), PL.golden_patient_table(HAND_P, HAND_Y, HAND_IDS)):
        assert tbl["Patient_ID"].tolist() == ["a", "b"]
        assert tbl["num_windows"].tolist() == [3, 2] and tbl["num_passes"].tolist() == [3, 3]
        np.testing.assert_allclose(tbl["hours"], [0.05, 2 / 60], rtol=1e-12)
        np.testing.assert_allclose(tbl["true_index"], [40.0, 0.0], rtol=1e-12)
        np.testing.assert_allclose(tbl["pred_index"], [20.0, 0.0], rtol=1e-12)
        assert tbl["true_severity"].tolist() == [3, 0] and tbl["pred_severity"].tolist() == [2, 0]
        np.testing.assert_allclose(tbl["index_mean"], [100 / 3, 10.0], rtol=1e-12)   # passes 40, 40, 20 | 0, 30, 0
        np.testing.assert_allclose(tbl["p_normal"], [0, 2 / 3], atol=1e-12)
        np.testing.assert_allclose(tbl["p_mild"], [0, 0], atol=1e-12)
        np.testing.assert_allclose(tbl["p_moderate"], [1 / 3, 0], atol=1e-12)
        np.testing.assert_allclose(tbl["p_severe"], [2 / 3, 1 / 3], atol=1e-12)      # 30 / h is severe
        h = -(1 / 3 * np.log(1 / 3) + 2 / 3 * np.log(2 / 3))
        np.testing.assert_allclose(tbl["severity_entropy"], [h, h], rtol=1e-12)
        assert tbl["severity_confident"].tolist() == [False, False]
        np.testing.assert_allclose(tbl["patient_accuracy"], [2 / 3, 1.0], rtol=1e-12)
        np.testing.assert_allclose(tbl["sensitivity"], [0.5, 0.0], rtol=1e-12)       # b has no positive window
        np.testing.assert_allclose(tbl["specificity"], [1.0, 1.0], rtol=1e-12)
    table = PL.patient_table(HAND_P, HAND_Y, HAND_IDS)
    for m in (PL.cohort_metrics(table), PL.golden_cohort(table, HAND_P, HAND_Y, HAND_IDS)):
        # errors -20 and 0: bias -10, sample sd sqrt(200)
        assert abs(m["index_mae"] - 10.0) < 1e-6 and abs(m["index_bias"] + 10.0) < 1e-6
        assert abs(m["index_loa_lower"] - (-10 - 1.96 * np.sqrt(200))) < 1e-5
        assert abs(m["index_loa_upper"] - (-10 + 1.96 * np.sqrt(200))) < 1e-5
        assert m["severity_accuracy"] == 0.5 and m["severity_within_one"] == 1.0
        # weights 1 - |i - j| / 3: observed (1 + 2/3) / 2, expected (1 + 1/3 + 0 + 2/3) / 4
        assert abs(m["severity_kappa_linear"] - 2 / 3) < 1e-12
        assert m["share_confident"] == 0.0 and np.isnan(m["severity_accuracy_confident"])
        assert m["ci_coverage"] == 1.0                                               # 40 in [21, 40] and 0 in [0, 28.5]
        assert abs(m["accuracy"] - 0.8) < 1e-12 and m["sensitivity"] == 0.5 and m["specificity"] == 1.0


def test_eager_path_matches_golden(seed2):
    probs, y, ids = seed2
    got = PL.patient_table(probs, y, ids)
    ref = PL.golden_patient_table(probs, y, ids)
    check_table(got, ref)
    assert got["true_severity"].nunique() >= 3 and 0 < got["severity_confident"].mean() < 1
    check_cohort(PL.cohort_metrics(got), PL.golden_cohort(ref, probs, y, ids), ref)
    tp, pp = got["true_severity"].to_numpy(), got["pred_severity"].to_numpy()
    conf = P.finalize(PL._point_sums(got.attrs["patient_record"].array, "cpu"), 60.0)["confusion"]
    np.testing.assert_array_equal(conf, np.histogram2d(tp, pp, bins=(np.arange(5), np.arange(5)))[0])


def test_table_matches_existing_aggregation(seed2):
    probs, y, ids = seed2
    got = PL.patient_table(probs, y, ids)
    old = aggregate_patient_uq_metrics(per_window_table(probs, y, ids), verbose=False)
    assert got["Patient_ID"].tolist() == old["Patient_ID"].tolist()
    for c in ("mean_variance", "mean_entropy", "patient_accuracy", "num_windows"):
        np.testing.assert_allclose(got[c], old[c], rtol=1e-5, err_msg=c)


def test_cluster_replicates_match_naive_gather(seed2):
    probs, y, ids = seed2
    n_boot, seed = 12, 7
    got = PL.cluster_bootstrap_metrics(probs, y, ids, n_bootstrap=n_boot, random_state=seed, parity=True)
    uniq = np.unique(ids)
    idx = M.parity_bootstrap_indices(len(uniq), n_boot, seed)
    w = M.per_window(probs)
    assert len(got) == n_boot and tuple(got[0]) == M.AGG_KEYS
    for b, row in enumerate(idx):
        ix = np.concatenate([np.flatnonzero(ids == uniq[k]) for k in row])
        ref = M.aggregates({k: v[ix] for k, v in w.items()}, y[ix])
        for k in M.AGG_KEYS:
            np.testing.assert_allclose(got[b][k], ref[k], rtol=1e-6, err_msg=f"{k} replicate {b}")
    ci = compute_confidence_intervals(got)
    assert ci["overall_mean_variance_ci_lower"] < ci["overall_mean_variance_ci_upper"]


@pytest.mark.parametrize("seed", [2025, 1, 2, 3])
def test_cluster_interval_is_wider_than_window_interval(seed):
    probs, y, ids = cohort(seed)
    key = "overall_mean_variance"
    win = compute_confidence_intervals(bootstrap_metrics(probs, y, n_bootstrap=200, random_state=seed, device="cpu"))
    clu = compute_confidence_intervals(PL.cluster_bootstrap_metrics(probs, y, ids, n_bootstrap=200, random_state=seed))
    w_win = win[f"{key}_ci_upper"] - win[f"{key}_ci_lower"]
    w_clu = clu[f"{key}_ci_upper"] - clu[f"{key}_ci_lower"]
    print(f"seed {seed}: cluster width {w_clu:.6f}, window width {w_win:.6f}, ratio {w_clu / w_win:.2f}")
    assert w_clu >= 2.0 * w_win


def test_unsorted_and_string_ids(seed2):
    probs, y, ids = seed2
    base = PL.patient_table(probs, y, ids)
    perm = np.random.RandomState(0).permutation(len(y))
    mixed = PL.patient_table(probs[:, perm], y[perm], ids[perm])
    # the integer sums of the same per-window rows are equal bit for bit in any order ...
    pt, yt = torch.from_numpy(probs), torch.from_numpy(y)
    m, code, tp = uq_ops.metrics_eager(pt), torch.from_numpy(ids.astype(np.int32)), torch.from_numpy(perm)
    whole, shuffled = P.reduce_eager(pt, m, yt, code, 40), P.reduce_eager(pt[:, tp], m[:, tp], yt[tp], code[tp], 40)
    assert torch.equal(whole[0], shuffled[0]) and torch.equal(whole[1], shuffled[1])
    # ... and so is the table, up to the fp32 rounding of the eager per-window rows, which torch sums in an
    # order that depends on a window's position (2^-23 relative per window)
    check_table(mixed, base.assign(mean_variance=mixed["mean_variance"], mean_entropy=mixed["mean_entropy"]))
    np.testing.assert_allclose(mixed["mean_variance"], base["mean_variance"], rtol=2.0 ** -22)
    np.testing.assert_allclose(mixed["mean_entropy"], base["mean_entropy"], rtol=2.0 ** -22)
    names = np.array([f"shhs1-{200000 + 7 * k}" for k in range(40)])
    named = PL.patient_table(probs, y, names[ids])
    order = np.argsort(names)                                      # np.unique sorts the strings
    assert named["Patient_ID"].tolist() == names[order].tolist()
    pd.testing.assert_frame_equal(named.drop(columns="Patient_ID"),
                                  base.iloc[order].drop(columns="Patient_ID").reset_index(drop=True))


def test_single_patient_and_single_window_patient():
    probs, y, ids = cohort(2)
    one = PL.patient_table(probs[:, :60], y[:60], np.zeros(60, dtype=np.int64))
    check_table(one, PL.golden_patient_table(probs[:, :60], y[:60], np.zeros(60)))
    m = PL.cohort_metrics(one)
    assert m["index_loa_lower"] == m["index_bias"] == m["index_loa_upper"]     # no spread with one patient
    assert np.isnan(m["pearson_r_accuracy_entropy"]) and m["severity_kappa_linear"] == 0.0
    res = PL.evaluate_patient_level(probs[:, :60], y[:60], np.zeros(60), "one", n_bootstrap=5, make_plots=False)
    assert res["index_mae_ci_lower"] == res["index_mae"] == res["index_mae_ci_upper"]
    assert np.isnan(res["pearson_r_accuracy_entropy_ci_lower"])
    ids2 = np.concatenate([[7], np.full(59, 3)])                   # patient 7 has one window
    two = PL.patient_table(probs[:, :60], y[:60], ids2)
    check_table(two, PL.golden_patient_table(probs[:, :60], y[:60], ids2))
    row = two[two["Patient_ID"] == 7].iloc[0]
    assert row["num_windows"] == 1 and row["true_index"] in (0.0, 60.0) and row["pred_index"] in (0.0, 60.0)


def test_single_pass(seed2):
    probs, y, ids = seed2
    mean = probs.mean(axis=0)
    t1 = PL.patient_table(mean, y, ids)                            # (N,): one pass
    check_table(t1, PL.golden_patient_table(mean, y, ids))
    assert (t1["num_passes"] == 1).all() and (t1["index_std"] == 0).all()
    np.testing.assert_array_equal(t1["index_ci_lower"], t1["pred_index"])
    np.testing.assert_array_equal(t1["index_ci_upper"], t1["pred_index"])
    assert t1["severity_confident"].all() and (t1["severity_entropy"] == 0).all()
    t3 = PL.patient_table(probs[:, :, None], y, ids)               # (T, N, 1)
    pd.testing.assert_frame_equal(t3, PL.patient_table(probs, y, ids))


def test_corner_probabilities():
    """p = 0, 0.5 and NaN are not positive, p = 1 is; a NaN metric adds 0 to the fixed-point sums."""
    p = np.array([[0.0, 0.5, 1.0, np.nan, 0.7, 0.2],
                  [0.0, 0.5, 1.0, 0.9, 0.8, 0.1]], dtype=np.float32)
    y = np.array([0, 1, 1, 1, 1, 0])
    code = torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.int32)
    pt = torch.from_numpy(p)
    m = uq_ops.metrics_eager(pt)
    pass_pos, rec = P.reduce_eager(pt, m, torch.from_numpy(y), code, 2)
    assert pass_pos.tolist() == [[1, 1], [2, 1]]
    assert rec[:, :5].tolist() == [[4, 3, 1, 1, 2], [2, 1, 1, 1, 2]]   # the NaN window is predicted 0
    ok = torch.tensor([True, True, True, False, True, True])
    _, rec_ok = P.reduce_eager(pt[:, ok], m[:, ok], torch.from_numpy(y)[ok], code[ok], 2)
    assert torch.equal(rec[:, 5:], rec_ok[:, 5:])
    assert rec[0, 5] == 0 and rec[0, 11] == P.Q_SCALE                  # variance 0; one bit from p = 0.5
    tbl = PL.patient_table(p, y, code.numpy())
    assert tbl["pred_index"].tolist() == [15.0, 30.0] and not tbl.isna().any().any()
    # codes outside [0, P) are skipped; shards add exactly
    bad = torch.tensor([0, -1, 0, 2, 1, 1], dtype=torch.int32)
    pp_bad, rec_bad = P.reduce_eager(pt, m, torch.from_numpy(y), bad, 2)
    keep = torch.tensor([True, False, True, False, True, True])
    pp_k, rec_k = P.reduce_eager(pt[:, keep], m[:, keep], torch.from_numpy(y)[keep], bad[keep], 2)
    assert torch.equal(pp_bad, pp_k) and torch.equal(rec_bad, rec_k)
    a = P.reduce_eager(pt[:, :2], m[:, :2], torch.from_numpy(y)[:2], code[:2], 2)
    b = P.reduce_eager(pt[:, 2:], m[:, 2:], torch.from_numpy(y)[2:], code[2:], 2)
    assert torch.equal(a[0] + b[0], pass_pos) and torch.equal(a[1] + b[1], rec)


def test_bootstrap_sums_eager_and_limits(seed2):
    probs, y, ids = seed2
    prec = torch.from_numpy(PL.patient_table(probs, y, ids).attrs["patient_record"].array)
    n_pat = prec.shape[0]
    assert prec.shape[1] == P.N_PREC == 25 and P.N_SUMS == 41
    idx = torch.from_numpy(M.parity_bootstrap_indices(n_pat, 6, 3).astype(np.int32))
    s = P.bootstrap_sums(prec, 6, idx=idx)
    for b in range(6):
        assert torch.equal(s[b, :25], prec[idx[b].long()].sum(0))
        assert int(s[b, 25:].sum()) == n_pat
    h = P.bootstrap_sums(prec, 6, seed=3)
    draws = uq_ops._hash_idx(n_pat, 6, 3, "cpu")                       # the keying of ops.uq.bootstrap with n = P
    assert torch.equal(h[:, :25], torch.stack([prec[d].sum(0) for d in draws]))
    big = prec.clone()
    big[0, 5] = (1 << 62)
    with pytest.raises(ValueError):
        P.bootstrap_sums(big, 1)
    with pytest.raises(ValueError):
        P.bootstrap_sums(prec[:, :24].contiguous(), 1)


def test_evaluate_patient_level_outputs(seed2, tmp_path):
    probs, y, ids = seed2
    res = PL.evaluate_patient_level(probs, y, ids, "unit", n_bootstrap=16, random_state=5, output_dir=str(tmp_path))
    for k in PL.COHORT_KEYS:
        assert res[f"{k}_ci_lower"] <= res[k] <= res[f"{k}_ci_upper"], k
    csv = pd.read_csv(tmp_path / "patient_severity_unit.csv")
    assert len(csv) == 40 and {"Patient_ID", "pred_index", "index_ci_lower", "p_severe", "severity_confident"} <= set(csv)
    if PL.plt is not None:
        assert (tmp_path / "bland_altman_unit.png").exists() and (tmp_path / "severity_confusion_unit.png").exists()
    with pytest.raises(ValueError):
        PL.cohort_metrics(csv)                                         # a table read back has no integer record
    with pytest.raises(ValueError):
        PL.patient_table(probs, y, ids[:-1])


def test_cli(tmp_path, seed2):
    assert "analyze_patient_severity" in commands.COMMANDS
    probs, y, ids = seed2
    per_window_table(probs, y, ids).to_csv(tmp_path / "detailed_results_X.csv", index=False)
    np.save(tmp_path / "mc_raw_pred_X.npy", probs[:, :, None])
    out1, out2 = tmp_path / "with_raw", tmp_path / "mean_only"
    t = commands.COMMANDS["analyze_patient_severity"](
        ["--input_csv", str(tmp_path / "detailed_results_X.csv"), "--raw_pred", str(tmp_path / "mc_raw_pred_X.npy"),
         "--n_bootstrap", "8", "--seed", "3", "--output_dir", str(out1), "--no_plots"])
    assert set(t["metric"]) == set(PL.COHORT_KEYS)
    a = pd.read_csv(out1 / "patient_severity_detailed_results_X.csv")
    assert len(a) == 40 and (a["num_passes"] == 20).all()
    assert os.path.exists(out1 / "patient_cohort_metrics_detailed_results_X.csv")
    commands.COMMANDS["analyze_patient_severity"](
        ["--input_csv", str(tmp_path / "detailed_results_X.csv"), "--n_bootstrap", "8", "--no_parity",
         "--window_seconds", "30", "--output_dir", str(out2), "--no_plots"])
    b = pd.read_csv(out2 / "patient_severity_detailed_results_X.csv")
    assert (b["num_passes"] == 1).all() and (b["index_ci_lower"] == b["index_ci_upper"]).all()
    np.testing.assert_allclose(b["true_index"], 2 * a["true_index"], rtol=1e-12)   # 30 s windows: twice per hour
