"""Rank statistics on the CPU: the integer emulation of the HIP kernels (``ops/rank.py``) and the public API
(``uq/discrimination.py``) against scikit-learn / SciPy on the literal resamples."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.analysis.stats import entropy_mannwhitney
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rank
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import discrimination as D
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M

from .rank_fixtures import STRUCTURES, TOL_PR, TOL_RANK, check_against_golden, make_scores

B = 12


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("n", [70, 257, 3001])
def test_scan_eager_matches_golden(n, structure):
    s, y = make_scores(n, structure)
    idx = M.parity_bootstrap_indices(n, B, 11)
    pr = rank.prep(torch.from_numpy(s), torch.from_numpy(y))
    assert pr["n_valid"] == n and pr["packed"].dtype == torch.uint8
    assert torch.equal(pr["pos"][pr["perm"]].long(), torch.arange(n))
    w = rank.weights_eager(pr["pos"], n, B, torch.from_numpy(idx.astype(np.int32)))
    assert torch.equal(w.sum(1), torch.full((B,), n))
    sums = rank.scan_sums_eager(w, pr["packed"])
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (B, 6)
    assert torch.equal(sums, rank.bootstrap_sums(pr, B, idx=torch.from_numpy(idx.astype(np.int32))))
    fin = rank.finalize(sums)
    gold = D.golden_replicates(s, y, idx)
    check_against_golden(fin, gold)
    assert np.array_equal(fin["n_pos"], gold["n_pos"]) and np.array_equal(fin["n_neg"], gold["n_neg"])
    if structure == "equal":
        assert np.all(fin["auroc"] == 0.5) and np.all(fin["groups"] == 1)
    # the point estimate: every window once
    one = rank.finalize(rank.scan_sums_eager(torch.ones(1, n, dtype=torch.int32), pr["packed"])[0])
    g1 = D.golden_discrimination(s, y)
    check_against_golden({k: np.array([v]) for k, v in one.items()}, {k: np.array([v]) for k, v in g1.items()})


def test_hash_weights_are_the_shared_resamples():
    """Without ``idx`` replicate b draws row b of the counter hash of the other analyses, whatever the chunk."""
    n, seed = 257, 7
    s, y = make_scores(n, "levels8")
    pr = rank.prep(torch.from_numpy(s), torch.from_numpy(y))
    idx = uq_ops._hash_idx(n, B, seed, "cpu")
    ref = rank.weights_eager(pr["pos"], n, B, idx.to(torch.int32))
    assert torch.equal(rank.weights_eager(pr["pos"], n, B, None, seed), ref)
    assert torch.equal(rank.weights_eager(pr["pos"], n, 5, None, seed, b0=4), ref[4:9])
    check_against_golden(rank.finalize(rank.bootstrap_sums(pr, B, seed=seed)), D.golden_replicates(s, y, idx.numpy()))


def test_one_class_replicates_and_zero_weight_groups():
    n = 70
    s, y = make_scores(n, "levels8")
    neg, pos = np.flatnonzero(y == 0), np.flatnonzero(y == 1)
    idx = np.stack([np.resize(neg, n), np.resize(pos, n), M.parity_bootstrap_indices(n, 1, 5)[0]])
    idx[2, :3] = [-1, n, n + 5]  # out-of-range draws are skipped
    pr = rank.prep(torch.from_numpy(s), torch.from_numpy(y))
    w = rank.weights_eager(pr["pos"], n, 3, torch.from_numpy(idx.astype(np.int32)))
    sums = rank.scan_sums_eager(w, pr["packed"])
    fin = rank.finalize(sums)
    assert sums[0].tolist()[:3] == [n, 0, 0] and sums[1].tolist()[:3] == [n, n, 0]
    assert int(sums[2, 0]) == n - 3
    assert int(sums[0, 3]) == len(np.unique(s[neg])) and int(sums[1, 3]) == len(np.unique(s[pos]))
    for k in ("auroc", "pr_auc", "average_precision"):
        assert np.isnan(fin[k][0]) and np.isnan(fin[k][1]) and not np.isnan(fin[k][2])
    assert fin["u_statistic"][0] == 0.0 and fin["u_statistic"][1] == 0.0
    assert fin["n_pos"].tolist()[:2] == [0, n] and fin["n_neg"].tolist()[:2] == [n, 0]
    gold = D.golden_replicates(s, y, idx[2:, 3:])
    check_against_golden({k: v[2:] for k, v in fin.items()}, gold)
    # groups of weight 0 are no curve points: the replicate equals the scan of its non-zero windows alone
    keep = w[2] > 0
    sub = rank.prep(pr["sorted"][keep], torch.from_numpy(y)[pr["perm"]][keep])
    assert torch.equal(rank.scan_sums_eager(w[2:3, keep].contiguous(), sub["packed"]), sums[2:3])


def test_non_finite_scores_are_dropped():
    n = 257
    s, y = make_scores(n, "continuous")
    s[[3, 50, 200]] = [np.nan, np.inf, -np.inf]
    pr = rank.prep(torch.from_numpy(s), torch.from_numpy(y))
    assert pr["n_valid"] == n - 3 and pr["n_total"] == n
    assert pr["pos"][[3, 50, 200]].tolist() == [-1, -1, -1]
    idx = M.parity_bootstrap_indices(n, B, 2)
    sums = rank.bootstrap_sums(pr, B, idx=torch.from_numpy(idx.astype(np.int32)))
    assert torch.equal(sums[:, 0], torch.from_numpy(np.isfinite(s[idx]).sum(1)))
    check_against_golden(rank.finalize(sums), D.golden_replicates(s, y, idx))
    probs = np.clip(s, 0, 1)
    probs[~np.isfinite(s)] = 0.5
    res = D.discrimination_metrics(probs, y, task="error", score=s)
    assert res["n_valid"] == n - 3 and res["n_pos"] + res["n_neg"] == n - 3


@pytest.fixture(scope="module")
def frame():
    rs = np.random.RandomState(5)
    n = 1500
    p = rs.rand(n).astype(np.float32)
    y = (rs.rand(n) < p).astype(np.int64)
    ent = np.round(M.binary_entropy_bits(p.astype(np.float64)) + 0.05 * rs.rand(n), 2)  # float64 with ties
    pids = np.repeat(np.arange(12), [40, 310, 75, 5, 160, 90, 220, 130, 61, 180, 29, 200])
    return pd.DataFrame({"Patient_ID": pids, "Window_Index": np.arange(n), "True_Label": y,
                         "Predicted_Label": (p > 0.5).astype(np.int64), "Predicted_Probability": p,
                         "Predictive_Variance": (rs.rand(n) * 0.1).astype(np.float32), "Predictive_Entropy": ent})


def test_error_task_is_entropy_mannwhitney(frame):
    from scipy.stats import mannwhitneyu

    p, y, ent = (frame[c].to_numpy() for c in ("Predicted_Probability", "True_Label", "Predictive_Entropy"))
    res = D.discrimination_metrics(p, y, task="error", score=ent)
    stat, _ = entropy_mannwhitney(frame, verbose=False)
    assert res["u_statistic"] == stat
    wrong = frame["Predicted_Label"].to_numpy() != y
    ref = mannwhitneyu(ent[wrong], ent[~wrong], alternative="greater", method="asymptotic")
    assert res["u_statistic"] == ref.statistic
    print(f"p-value {res['p_value']:.17g} scipy {ref.pvalue:.17g}")
    assert 0 < ref.pvalue < 1 and abs(res["p_value"] - ref.pvalue) <= 1e-12 * ref.pvalue
    assert res["n_pos"] == int(wrong.sum()) and res["n_neg"] == int((~wrong).sum())
    # task "apnea": the quantities of classification_metrics
    from sklearn.metrics import roc_auc_score

    ap = D.discrimination_metrics(p, y, task="apnea")
    assert abs(ap["auroc"] - roc_auc_score(y, p.astype(np.float64))) <= TOL_RANK


def test_cluster_bootstrap_matches_literal_golden(frame):
    p, y, ent, pids = (frame[c].to_numpy() for c in ("Predicted_Probability", "True_Label", "Predictive_Entropy",
                                                     "Patient_ID"))
    seed = 9
    uniq = np.unique(pids)
    assert len(uniq) == 12
    draws = M.parity_bootstrap_indices(len(uniq), B, seed)   # the draws of cluster_bootstrap_metrics
    win = [np.flatnonzero(pids == u) for u in uniq]
    wrong = ((p > 0.5).astype(np.int64) != y).astype(np.int64)
    for task, s, t in (("apnea", p.astype(np.float64), y), ("error", ent, wrong)):
        gold = [D.golden_discrimination(s[ix], t[ix]) for ix in (np.concatenate([win[d] for d in row]) for row in draws)]
        gold = {k: np.array([g[k] for g in gold]) for k in gold[0]}
        rep = D.discrimination_replicates(p, y, task=task, score=ent, n_bootstrap=B, random_state=seed, patient_ids=pids)
        check_against_golden(rep, gold)
        assert np.array_equal(rep["n_pos"], gold["n_pos"])
    res = D.evaluate_discrimination(p, y, "unit", n_bootstrap=B, random_state=seed, patient_ids=pids, score=ent,
                                    make_plots=False)
    assert abs(res["error_auroc_ci_lower"] - np.percentile(gold["auroc"], 2.5)) <= TOL_RANK
    # hash draws: another stream of patients, the same point values
    res_h = D.evaluate_discrimination(p, y, "unit", n_bootstrap=B, random_state=seed, patient_ids=pids, score=ent,
                                      parity=False, make_plots=False)
    assert res_h["apnea_auroc"] == res["apnea_auroc"] and res_h["apnea_auroc_mean"] != res["apnea_auroc_mean"]


def test_evaluate_discrimination(frame, tmp_path):
    p, y, ent = (frame[c].to_numpy() for c in ("Predicted_Probability", "True_Label", "Predictive_Entropy"))
    out = str(tmp_path / "plots")
    res = D.evaluate_discrimination(p, y, "unit", n_bootstrap=B, random_state=2025, score=ent, output_plot_dir=out)
    keys = {f"{t}_{k}" for t in D.TASKS for k in D.METRICS + ("p_value", "n_pos", "n_neg", "n_valid")}
    keys |= {f"{t}_{k}{e}" for t in D.TASKS for k in D.METRICS for e in ("_mean", "_ci_lower", "_ci_upper")}
    assert set(res) == keys
    idx = M.parity_bootstrap_indices(len(p), B, 2025)
    gold = D.golden_replicates(p.astype(np.float64), y, idx)
    for k, tol in (("auroc", TOL_RANK), ("pr_auc", TOL_PR), ("average_precision", TOL_PR)):
        assert abs(res[f"apnea_{k}"] - D.golden_discrimination(p, y)[k]) <= tol
        assert abs(res[f"apnea_{k}_mean"] - np.mean(gold[k])) <= tol
        assert abs(res[f"apnea_{k}_ci_lower"] - np.percentile(gold[k], 2.5)) <= tol
        assert abs(res[f"apnea_{k}_ci_upper"] - np.percentile(gold[k], 97.5)) <= tol
    if D.plt is not None:
        for name in ("roc_apnea_unit.png", "pr_apnea_unit.png", "roc_error_unit.png", "pr_error_unit.png"):
            assert os.path.exists(os.path.join(out, name))


def test_compare_is_paired(frame):
    rs = np.random.RandomState(8)
    pa = frame["Predicted_Probability"].to_numpy()
    y = frame["True_Label"].to_numpy()
    pb = np.clip(pa + 0.3 * (rs.rand(len(pa)).astype(np.float32) - 0.5), 0, 1)
    kw = dict(n_bootstrap=B, random_state=4)
    cmp, reps = D.compare_discrimination(pa, pb, y, return_replicates=True, **kw)
    for task in D.TASKS:
        ra = D.discrimination_replicates(pa, y, task=task, **kw)
        rb = D.discrimination_replicates(pb, y, task=task, **kw)
        for k in D.METRICS:
            assert np.array_equal(reps[f"{task}_{k}"], ra[k] - rb[k]), (task, k)
            d = ra[k] - rb[k]
            assert cmp[f"{task}_{k}_diff_ci_lower"] == float(np.percentile(d, 2.5))
            assert cmp[f"{task}_{k}_share_a_gt_b"] == float(np.mean(d > 0))
    assert cmp["apnea_auroc_diff"] == cmp["apnea_auroc_a"] - cmp["apnea_auroc_b"] > 0   # noise hurts
    assert cmp["apnea_auroc_share_a_gt_b"] == 1.0


def test_limits_raise():
    s, y = make_scores(70, "continuous")
    pr = rank.prep(torch.from_numpy(s), torch.from_numpy(y))
    with pytest.raises(ValueError):
        rank.prep(torch.zeros(5), torch.zeros(4))
    with pytest.raises(ValueError):   # more than 2^27 windows (a zero-stride view: no memory behind it)
        rank.weights_eager(torch.zeros(1, dtype=torch.int32).expand(rank.MAX_N + 1), 1, 1)
    with pytest.raises(ValueError):
        rank.scan_sums(torch.zeros(1, dtype=torch.int32).expand(1, rank.MAX_N + 1), pr["packed"])
    w = torch.zeros(1, 70, dtype=torch.int32)
    w[0, :2] = 1 << 30     # total weight 2^31
    with pytest.raises(ValueError):
        rank.scan_sums_eager(w, pr["packed"])
    w[0, 0] = -1
    with pytest.raises(ValueError):
        rank.scan_sums_eager(w, pr["packed"])
    with pytest.raises(ValueError):
        rank.scan_sums_eager(w.long(), pr["packed"])
    with pytest.raises(ValueError):
        rank.split_bounds(pr["packed"], rank.MAX_SPLITS + 1)
    with pytest.raises(ValueError):   # P patients x largest patient >= 2^31
        rank.check_cluster_limit(1 << 16, 1 << 15)
    rank.check_cluster_limit(1 << 15, (1 << 16) - 1)
    with pytest.raises(ValueError):
        D.discrimination_metrics(s, y, task="other")
    with pytest.raises(ValueError):
        D.evaluate_discrimination(s, y, patient_ids=np.zeros(3), make_plots=False)
    assert rank.S_BITS == 56 and rank.MAX_N * 2.0 ** -(rank.S_BITS + 1) <= 1e-9
    assert rank.chunk_replicates(rank.MAX_N) == 1 and rank.chunk_replicates(1 << 20) == 64


def test_split_bounds_are_group_starts():
    s, y = make_scores(3001, "levels8")
    pr = rank.prep(torch.from_numpy(s), torch.from_numpy(y))
    start = (pr["packed"] & rank.START_BIT) != 0
    for g in (1, 2, 8, 64):
        b = rank.split_bounds(pr["packed"], g).long()
        assert b.dtype == torch.int64 and b.numel() == g + 1 and int(b[0]) == 0 and int(b[-1]) == 3001
        assert bool((b[1:] >= b[:-1]).all()) and bool(start[b[:-1]].all())


def test_cli(frame, tmp_path):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import commands

    rs = np.random.RandomState(2)
    other = frame.copy()
    other["Predicted_Probability"] = np.clip(frame["Predicted_Probability"] + 0.3 * (rs.rand(len(frame)) - 0.5), 0, 1)
    other["Predicted_Label"] = (other["Predicted_Probability"] > 0.5).astype(int)
    src, cmp, dst = str(tmp_path / "detail.csv"), str(tmp_path / "other.csv"), str(tmp_path / "out" / "disc.csv")
    frame.to_csv(src, index=False)
    other.to_csv(cmp, index=False)
    assert "analyze_discrimination" in commands.COMMANDS
    commands.main(["analyze_discrimination", "--input_csv", src, "--score", "Predictive_Entropy", "--cluster",
                   "--compare_csv", cmp, "--n_bootstrap", "8", "--seed", "1", "--output_csv", dst, "--no_plots"])
    t = pd.read_csv(dst).set_index("metric")
    assert list(t.columns) == ["value", "mean", "ci_lower", "ci_upper"]
    assert {"apnea_auroc", "error_auroc", "error_u_statistic", "error_p_value", "apnea_pr_auc_diff",
            "apnea_auroc_share_a_gt_b"} <= set(t.index)
    row = t.loc["apnea_auroc"]
    assert row["ci_lower"] <= row["mean"] <= row["ci_upper"]
    stat, _ = entropy_mannwhitney(frame, verbose=False)
    assert t.loc["error_u_statistic", "value"] == stat
    assert t.loc["apnea_auroc_diff", "value"] > 0 and t.loc["apnea_auroc_diff", "ci_lower"] > 0
    # window bootstrap of the same file: same point values, narrower or different interval
    dst2 = str(tmp_path / "out" / "disc_w.csv")
    commands.main(["analyze_discrimination", "--input_csv", src, "--n_bootstrap", "8", "--seed", "1", "--output_csv", dst2,
                   "--no_plots"])
    t2 = pd.read_csv(dst2).set_index("metric")
    assert t2.loc["apnea_auroc", "value"] == row["value"] and t2.loc["apnea_auroc", "ci_lower"] != row["ci_lower"]
