"""Command-line entry points mirroring every reference script (same flag names and defaults).

``python -m uncertaintyquantification_sleepapnea_1dcnn_amd <command> [flags]`` or
``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.<command> [flags]``.

| command | reference script |
|---|---|
| preprocess_shhs_raw | data_prepocessing/preprocess_shhs_raw.py |
| prepare_numpy_datasets | data_prepocessing/prepare_numpy_datasets.py |
| cnn_baseline_train | models/cnn_baseline_train.py |
| train_deep_ensemble_cnns | models/train_deep_ensemble_cnns.py (torchrun: one member per GPU) |
| analyze_mcd_patient_level | uncertainty_quantification/analyze_mcd_patient_level.py |
| analyze_de_patient_level | uncertainty_quantification/analyze_de_patient_level.py |
| evaluate_mcd_global | uncertainty_quantification/evaluate_mcd_global.py |
| evaluate_de_global | uncertainty_quantification/evaluate_de_global.py |
| aggregate_patient_uq_metrics | uncertainty_quantification/aggregate_patient_uq_metrics.py |
| analyze_window_level_uncertainty | uncertainty_quantification/analyze_window_level_uncertainty.py |
| final_plot_uq_overview_figures | uq_analysis/final_plot_uq_overview_figures.py |
| patient_accuracy_entropy_correlation | uq_analysis/patient_accuracy_entropy_correlation.py |
| window_uncertainty_vs_correctness_mannwhitney | uq_analysis/window_uncertainty_vs_correctness_mannwhitney.py |
| hyperparameter_plot_mcd_or_de_pass_convergence | uq_analysis/hyperparameter_plot_mcd_or_de_pass_convergence.py |
| convergence_sweep | (new) computes the convergence CSV the reference produced by hand |
| shhs_cohort_analysis / shhs_signal_quality | datasets/SHHS_cohort_analysis.py / SHHS_signal_quality.py |
| uq_demo | uq_techniques.py ``__main__`` demo |
| analyze_calibration | (new) calibration + selective prediction with bootstrap CIs from a detail CSV |
| analyze_patient_severity | (new) per-patient apnea index, severity and cohort metrics with patient-cluster bootstrap CIs |
| analyze_pass_convergence | (new) how many passes / members are enough: every metric against the count, with bands over random subsets, from one raw prediction dump |
| analyze_laplace_patient_level | (new) last-layer Laplace UQ evaluation with per-window results: fits (or loads) the posterior of the Dense head, then the outputs of analyze_mcd_patient_level |
| analyze_discrimination | (new) ROC / PR AUC and Mann-Whitney U (apnea vs normal, wrong vs right predictions) with window or patient-cluster bootstrap CIs, and the paired comparison of two detail CSVs |
| analyze_recalibration | (new) temperature / Platt / beta recalibration of a raw prediction dump (fit set or patient cross-fit): calibration before and after on the same resamples, and the calibrated (T, N, 1) dump for the other analyze_* commands |
| analyze_conformal | (new) split conformal prediction sets from a detail CSV: thresholds from a fit CSV and the set code of every window, or coverage / set sizes over random calibration / test splits of the patients |
| analyze_shift_robustness | (new) one sampler (MC Dropout, Deep Ensemble, Laplace) on degraded, re-standardised copies of the test windows: accuracy, calibration, uncertainty, detection AUROC and conformal coverage per (corruption, severity), and one figure per corruption |
| analyze_ensemble_members | (new) ensemble composition from one raw prediction dump: every member alone and leave-one-out, pairwise diversity, greedy pruning cross-fitted by patient against first-k and random-k, and the pruned (k, N, 1) dump for the other analyze_* commands |
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

SEED = 2025


def preprocess_shhs_raw(argv=None):
    from ..data.preprocess import main

    main(argv)


def prepare_numpy_datasets(argv=None):
    from ..data.prepare import main

    main(argv)


def cnn_baseline_train(argv=None):
    from ..training.experiment import main

    main(argv)


def train_deep_ensemble_cnns(argv=None):
    ap = argparse.ArgumentParser(description="Train CNN ensemble models (member-parallel over GPUs under torchrun).")
    ap.add_argument("--model_type", type=str, default="cnn", help="Type of model to train (only 'cnn' supported).")
    ap.add_argument("--num_models", type=int, default=5)
    ap.add_argument("--seed_base", type=int, default=SEED)
    ap.add_argument("--data_dir", type=str, default="./processed_datasets")
    ap.add_argument("--save_dir", type=str, default="./models/ensemble_cnn_no_pool")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch_size", type=int, default=1024)
    ap.add_argument("--patience", type=int, default=5)
    ap.add_argument("--name_offset", type=int, default=21)
    a = ap.parse_args(argv)
    if a.model_type.lower() != "cnn":
        print(f"Error: This script is configured to train only 'cnn' models, but received '{a.model_type}'.")
        return
    from ..data.prepare import load_processed
    from ..parallel.ensemble import train_ensemble

    X = load_processed(a.data_dir, "X_train_win_std_smote.npy")
    y = load_processed(a.data_dir, "y_train_smote.npy").astype(np.float32)
    train_ensemble(X, y, a.num_models, a.seed_base, a.save_dir, name_offset=a.name_offset, epochs=a.epochs,
                   batch_size=a.batch_size, patience=a.patience)


def reference_train_ensemble(model_type: str = "cnn", num_models: int = 5, seed_base: int = SEED,
                             data_dir: str = "./processed_datasets", save_dir: str = "./models/ensemble_cnn_no_pool"):
    """``train_deep_ensemble_cnns.py:81`` signature ``train_ensemble(model_type, num_models, seed_base)``:
    loads the SMOTE training set from ``data_dir`` and trains the members (skip-if-exists resume)."""
    argv = ["--model_type", model_type, "--num_models", str(num_models), "--seed_base", str(seed_base),
            "--data_dir", data_dir, "--save_dir", save_dir]
    train_deep_ensemble_cnns(argv)


def _load_test(data_dir):
    from ..data.prepare import load_processed

    Xu = load_processed(data_dir, "X_test_win_std_unbalanced.npy")
    yu = load_processed(data_dir, "y_test_unbalanced.npy")
    try:
        pids = load_processed(data_dir, "patient_ids_test_unbalanced.npy")
    except FileNotFoundError:
        pids = None
    Xr = load_processed(data_dir, "X_test_win_std_rus.npy")
    yr = load_processed(data_dir, "y_test_rus.npy")
    return Xu, yu, pids, Xr, yr


def _uq_common(ap):
    ap.add_argument("--data_dir", type=str, default="./processed_datasets")
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--no_plots", action="store_true")


def analyze_mcd_patient_level(argv=None, global_mode: bool = False):
    ap = argparse.ArgumentParser(description="MC Dropout UQ evaluation with per-window results.")
    _uq_common(ap)
    ap.add_argument("--model_path", type=str, default="./AlCNN1D_no_pool.keras")
    ap.add_argument("--n_passes", type=int, default=50)
    ap.add_argument("--bn_mode", choices=["batch", "running"], default="batch",
                    help="batch = reference semantics (model(x, training=True)); running = standard MC Dropout")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots_patient/mc_dropout_no_pool")
    ap.add_argument("--output_csv_dir", type=str, default="./uq_results_patient_no_pool")
    a = ap.parse_args(argv)
    from ..models.cnn import load_model
    from ..uq.drivers import evaluate_mc_dropout

    np.random.seed(a.seed)
    Xu, yu, pids, Xr, yr = _load_test(a.data_dir)
    model = load_model(a.model_path)
    det = model.predict(Xu)
    print(f"Deterministic Accuracy (training=False) on Unbalanced Set: {np.mean((det.ravel() > 0.5) == yu):.4f}")
    res = {}
    res["unbalanced"] = evaluate_mc_dropout(model, Xu, yu, None if global_mode else pids,
                                            "CNN_MCD_Unbalanced", not global_mode, a.n_passes, a.n_bootstrap, a.seed,
                                            a.bn_mode, a.output_csv_dir, a.output_plot_dir,
                                            raw_pred_path="./mc_raw_pred0205.npy" if global_mode else None,
                                            make_plots=not a.no_plots)
    res["balanced"] = evaluate_mc_dropout(model, Xr, yr, None, "CNN_MCD_Balanced_RUS", False, a.n_passes, a.n_bootstrap,
                                          a.seed, a.bn_mode, a.output_csv_dir, a.output_plot_dir, raw_pred_path="",
                                          make_plots=not a.no_plots)
    return res


def evaluate_mcd_global(argv=None):
    return analyze_mcd_patient_level(argv, global_mode=True)


def _load_named(data_dir, name, mmap=False):
    """A ``.npy`` given as a path, or as a processed-dataset name under ``data_dir`` (FILE_ALIASES honoured)."""
    from ..data.prepare import load_processed

    if os.path.exists(name):
        return np.load(name, mmap_mode="r" if mmap else None, allow_pickle=False)
    return load_processed(data_dir, name, mmap=mmap)


def analyze_laplace_patient_level(argv=None):
    ap = argparse.ArgumentParser(description="Last-layer Laplace UQ evaluation with per-window results: one trained "
                                             "model, one deterministic pass, draws of the Dense head.")
    _uq_common(ap)
    ap.add_argument("--model_path", type=str, default="./AlCNN1D_no_pool.keras")
    ap.add_argument("--fit_x", type=str, default="X_train_win_std_smote.npy",
                    help="training windows (.npy path, or a processed-dataset name under --data_dir)")
    ap.add_argument("--fit_y", type=str, default="y_train_smote.npy", help="training labels (as --fit_x)")
    ap.add_argument("--prior_precision", type=str, default="auto", help="'auto' (evidence maximisation) or a float")
    ap.add_argument("--n_samples", type=int, default=50)
    ap.add_argument("--state", type=str, default="./laplace_state.npz",
                    help="posterior file: loaded if present, else fitted on --fit_x / --fit_y and saved")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots_patient/laplace_no_pool")
    ap.add_argument("--output_csv_dir", type=str, default="./uq_results_patient_laplace")
    a = ap.parse_args(argv)
    from ..models.cnn import load_model
    from ..uq.drivers import evaluate_laplace
    from ..uq.laplace import LaplaceState, fit_laplace

    np.random.seed(a.seed)
    prior = a.prior_precision if a.prior_precision == "auto" else float(a.prior_precision)
    Xu, yu, pids, Xr, yr = _load_test(a.data_dir)
    model = load_model(a.model_path)
    det = model.predict(Xu)
    print(f"Deterministic Accuracy (training=False) on Unbalanced Set: {np.mean((det.ravel() > 0.5) == yu):.4f}")
    if os.path.exists(a.state):
        state = LaplaceState.load(a.state)
        print(f"Loaded the Laplace posterior from {a.state} (prior precision {state.prior_precision:.6g})")
    else:
        state = fit_laplace(model, _load_named(a.data_dir, a.fit_x, mmap=True), _load_named(a.data_dir, a.fit_y), prior)
        d = os.path.dirname(a.state)
        if d:
            os.makedirs(d, exist_ok=True)
        print(f"Fitted the Laplace posterior on {state.n_valid} of {state.n_total} windows (prior precision "
              f"{state.prior_precision:.6g}, log evidence {state.log_evidence:.4f}); saved to {state.save(a.state)}")
    res = {}
    res["unbalanced"] = evaluate_laplace(model, state, Xu, yu, pids, "CNN_LLLA_Unbalanced", True, a.n_samples,
                                         a.n_bootstrap, a.seed, a.output_csv_dir, a.output_plot_dir,
                                         make_plots=not a.no_plots)
    res["balanced"] = evaluate_laplace(model, state, Xr, yr, None, "CNN_LLLA_Balanced_RUS", False, a.n_samples,
                                       a.n_bootstrap, a.seed, a.output_csv_dir, a.output_plot_dir, raw_pred_path="",
                                       make_plots=not a.no_plots)
    return res


def analyze_de_patient_level(argv=None):
    ap = argparse.ArgumentParser(description="Deep Ensemble UQ evaluation with per-window results.")
    _uq_common(ap)
    ap.add_argument("--model_dir", type=str, default="./models/ensemble_cnn_no_pool")
    ap.add_argument("--pattern", type=str, default="AlCNN_smote_seed{}.keras")
    ap.add_argument("--num_members", type=int, default=5)
    ap.add_argument("--offset", type=int, default=5, help="file index of member 0 (reference loader uses i+5)")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots_patient/deep_ensemble_no_pool")
    ap.add_argument("--output_csv_dir", type=str, default="./uq_results_patient_DE_new")
    a = ap.parse_args(argv)
    from ..parallel.ensemble import load_ensemble
    from ..uq.drivers import evaluate_deep_ensemble

    np.random.seed(a.seed)
    Xu, yu, pids, Xr, yr = _load_test(a.data_dir)
    models = load_ensemble(a.model_dir, a.pattern, a.num_members, a.offset)
    return {"unbalanced": evaluate_deep_ensemble(models, Xu, yu, pids, "CNN_DE_Unbalanced", True, a.n_bootstrap, a.seed,
                                                 a.output_csv_dir, a.output_plot_dir, make_plots=not a.no_plots),
            "balanced": evaluate_deep_ensemble(models, Xr, yr, None, "CNN_DE_Balanced_RUS", False, a.n_bootstrap, a.seed,
                                               a.output_csv_dir, a.output_plot_dir, make_plots=not a.no_plots)}


def evaluate_de_global(argv=None):
    ap = argparse.ArgumentParser(description="Deep Ensemble global UQ evaluation (M=20 by default).")
    _uq_common(ap)
    ap.add_argument("--model_prefix", type=str, default="./models/ensemble_cnn/AlCNN_smote_seed")
    ap.add_argument("--num_models", type=int, default=20)
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots/deep_ensemble20")
    a = ap.parse_args(argv)
    from ..parallel.ensemble import load_ensemble_prefix
    from ..uq.drivers import evaluate_deep_ensemble

    Xu, yu, _, Xr, yr = _load_test(a.data_dir)
    models = load_ensemble_prefix(a.model_prefix, a.num_models)
    return {"unbalanced": evaluate_deep_ensemble(models, Xu, yu, None, "CNN_DE_Unbalanced", False, a.n_bootstrap, a.seed,
                                                 output_plot_dir=a.output_plot_dir, make_plots=not a.no_plots),
            "balanced": evaluate_deep_ensemble(models, Xr, yr, None, "CNN_DE_Balanced_RUS", False, a.n_bootstrap, a.seed,
                                               output_plot_dir=a.output_plot_dir, make_plots=not a.no_plots)}


def aggregate_patient_uq_metrics(argv=None):
    ap = argparse.ArgumentParser(description="Patient-level aggregation of per-window UQ results.")
    ap.add_argument("--input_csv", type=str, default="./detail_patient_MCD.csv")
    ap.add_argument("--output_dir", type=str, default="./patient_level_uq_analysis_MCD")
    ap.add_argument("--tag", type=str, default="MCD")
    a = ap.parse_args(argv)
    from ..analysis.patient import aggregate_patient_uq_metrics as f

    return f(a.input_csv, a.output_dir, a.tag)


def analyze_window_level_uncertainty(argv=None):
    ap = argparse.ArgumentParser(description="Window-level uncertainty vs correctness (binned accuracy).")
    ap.add_argument("--input_csv", type=str, default="./detail_patient_DE.csv")
    ap.add_argument("--num_bins", type=int, default=10)
    a = ap.parse_args(argv)
    from ..analysis.patient import window_level_binning

    return window_level_binning(a.input_csv, num_bins=a.num_bins)


def final_plot_uq_overview_figures(argv=None):
    ap = argparse.ArgumentParser(description="Thesis overview figures (MCD vs DE).")
    ap.add_argument("--mcd_detail", default="./detail_patient_MCD.csv")
    ap.add_argument("--de_detail", default="./detail_patient_DE.csv")
    ap.add_argument("--mcd_summary", default="./patient_level_uq_analysis_MCD/patient_summary_metrics_MCD.csv")
    ap.add_argument("--de_summary", default="./patient_level_uq_analysis_DE/patient_summary_metrics_DE.csv")
    ap.add_argument("--output_dir", default="./final_thesis_plots")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..analysis.figures import final_overview_figures

    ld = lambda p: pd.read_csv(p) if os.path.exists(p) else None  # noqa: E731
    return final_overview_figures(ld(a.mcd_detail), ld(a.de_detail), ld(a.mcd_summary), ld(a.de_summary), a.output_dir)


def patient_accuracy_entropy_correlation(argv=None):
    ap = argparse.ArgumentParser(description="Pearson correlation of patient mean entropy vs accuracy.")
    ap.add_argument("--mcd_csv", default="./patient_level_uq_analysis_MCD/patient_summary_metrics_MCD.csv")
    ap.add_argument("--de_csv", default="./patient_level_uq_analysis_DE/patient_summary_metrics_DE.csv")
    a = ap.parse_args(argv)
    from ..analysis.stats import patient_correlation

    out = {}
    for name, p in (("MC Dropout", a.mcd_csv), ("Deep Ensemble", a.de_csv)):
        if os.path.exists(p):
            out[name] = patient_correlation(p, name)
        else:
            print(f"ERROR: File not found - {p}")
    return out


def window_uncertainty_vs_correctness_mannwhitney(argv=None):
    ap = argparse.ArgumentParser(description="One-sided Mann-Whitney U: entropy of incorrect > correct windows.")
    ap.add_argument("--input_csv", default="./detail_patient_DE.csv")
    ap.add_argument("--method", default="Deep Ensembles")
    a = ap.parse_args(argv)
    from ..analysis.stats import entropy_mannwhitney

    return entropy_mannwhitney(a.input_csv, a.method)


def hyperparameter_plot_mcd_or_de_pass_convergence(argv=None):
    ap = argparse.ArgumentParser(description="Plot overall mean variance convergence vs passes/members.")
    ap.add_argument("--input_csv", type=str, default="")
    ap.add_argument("--output_plot", type=str, default="variance_convergence_plot.png")
    ap.add_argument("--method", type=str, default="mcd", choices=["mcd", "de"])
    a = ap.parse_args(argv)
    if not a.input_csv:
        print("ERROR: --input_csv is required")
        return None
    from ..analysis.figures import plot_variance_convergence

    return plot_variance_convergence(a.input_csv, a.output_plot, a.method)


def convergence_sweep(argv=None):
    ap = argparse.ArgumentParser(description="Compute the variance-convergence CSV for MCD passes or DE members.")
    ap.add_argument("--method", choices=["mcd", "de"], default="mcd")
    ap.add_argument("--data_dir", default="./processed_datasets")
    ap.add_argument("--model_path", default="./AlCNN1D_no_pool.keras")
    ap.add_argument("--model_dir", default="./models/ensemble_cnn_no_pool")
    ap.add_argument("--pattern", default="AlCNN_smote_seed{}.keras")
    ap.add_argument("--offset", type=int, default=5)
    ap.add_argument("--counts", default="5,10,20,30,40,50")
    ap.add_argument("--bn_mode", choices=["batch", "running"], default="running")
    ap.add_argument("--output_csv", default="./convergence_mcd.csv")
    a = ap.parse_args(argv)
    from ..uq import uq_techniques as U
    from ..uq.drivers import convergence_sweep as sweep

    Xu, yu, _, Xr, yr = _load_test(a.data_dir)
    counts = [int(c) for c in a.counts.split(",")]
    if a.method == "mcd":
        from ..models.cnn import load_model

        m = load_model(a.model_path)
        fn = lambda X, n: U.mc_dropout_predict(m, X, n, bn_mode=a.bn_mode)  # noqa: E731
    else:
        from ..parallel.ensemble import load_ensemble

        models = load_ensemble(a.model_dir, a.pattern, max(counts), a.offset)
        fn = lambda X, n: U.deep_ensembles_predict(models[:n], X)  # noqa: E731
    return sweep(fn, counts, Xu, yu, Xr, yr, a.output_csv)


def shhs_cohort_analysis(argv=None):
    from ..data.cohort import main_cohort

    main_cohort(argv)


def shhs_signal_quality(argv=None):
    from ..data.cohort import main_quality

    main_quality(argv)


def analyze_calibration(argv=None):
    ap = argparse.ArgumentParser(description="Calibration (ECE/MCE/Brier/NLL) and selective prediction "
                                             "(accuracy vs coverage) of a per-window detail CSV, with bootstrap CIs.")
    ap.add_argument("--input_csv", type=str, default="./detail_patient_DE.csv")
    ap.add_argument("--score", choices=["Predictive_Entropy", "Predictive_Variance"], default="Predictive_Entropy",
                    help="uncertainty column by which windows are referred")
    ap.add_argument("--n_bins", type=int, default=15)
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots/calibration")
    ap.add_argument("--output_csv", type=str, default="./calibration_metrics.csv")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..uq.calibration import evaluate_calibration

    df = pd.read_csv(a.input_csv)
    label = os.path.splitext(os.path.basename(a.input_csv))[0]
    res = evaluate_calibration(df["Predicted_Probability"].to_numpy(np.float32), df["True_Label"].to_numpy(), label,
                               n_bootstrap=a.n_bootstrap, random_state=a.seed,
                               score=df[a.score].to_numpy(np.float32), n_bins=a.n_bins,
                               output_plot_dir=a.output_plot_dir, make_plots=not a.no_plots)
    ends = ("_mean", "_ci_lower", "_ci_upper")
    rows = [{"metric": k, "value": v, "mean": res.get(k + "_mean", np.nan), "ci_lower": res.get(k + "_ci_lower", np.nan),
             "ci_upper": res.get(k + "_ci_upper", np.nan)} for k, v in res.items() if not k.endswith(ends)]
    table = pd.DataFrame(rows, columns=["metric", "value", "mean", "ci_lower", "ci_upper"])
    print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
    if a.output_csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.output_csv)), exist_ok=True)
        table.to_csv(a.output_csv, index=False)
    return table


def analyze_patient_severity(argv=None):
    ap = argparse.ArgumentParser(description="Per-patient window apnea index and severity with uncertainty, and cohort "
                                             "metrics with patient-cluster bootstrap CIs, from a per-window detail CSV.")
    ap.add_argument("--input_csv", type=str, default="./detailed_results_MCD.csv",
                    help="per-window CSV with Patient_ID, True_Label and Predicted_Probability")
    ap.add_argument("--raw_pred", type=str, default=None,
                    help="(T, N, 1) .npy dump of the passes (mc_raw_pred*.npy); without it the mean prediction is the "
                         "only pass")
    ap.add_argument("--window_seconds", type=float, default=60.0)
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--no_parity", action="store_true", help="draw patients with the device counter hash")
    ap.add_argument("--output_dir", type=str, default="./uq_plots/patient_severity")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..uq.patient_level import COHORT_KEYS, evaluate_patient_level

    df = pd.read_csv(a.input_csv)
    label = os.path.splitext(os.path.basename(a.input_csv))[0]
    if a.raw_pred:
        pred = np.load(a.raw_pred).astype(np.float32)
        n = pred.shape[1] if pred.ndim >= 2 else pred.shape[0]
        if n != len(df):
            raise ValueError(f"{a.raw_pred} holds {n} windows, {a.input_csv} {len(df)}")
    else:
        pred = df["Predicted_Probability"].to_numpy(np.float32)
        print("No --raw_pred: one pass (the mean prediction); the credible intervals are points (num_passes = 1).")
    res = evaluate_patient_level(pred, df["True_Label"].to_numpy(), df["Patient_ID"].to_numpy(), label,
                                 n_bootstrap=a.n_bootstrap, random_state=a.seed, parity=not a.no_parity,
                                 output_dir=a.output_dir, make_plots=not a.no_plots, window_seconds=a.window_seconds)
    rows = [{"metric": k, "value": res[k], "ci_lower": res.get(k + "_ci_lower", np.nan),
             "ci_upper": res.get(k + "_ci_upper", np.nan)} for k in COHORT_KEYS]
    table = pd.DataFrame(rows, columns=["metric", "value", "ci_lower", "ci_upper"])
    print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
    table.to_csv(os.path.join(a.output_dir, f"patient_cohort_metrics_{label}.csv"), index=False)
    print(f"Saved patient table to: {os.path.join(a.output_dir, f'patient_severity_{label}.csv')}")
    return table


def analyze_pass_convergence(argv=None):
    ap = argparse.ArgumentParser(description="Convergence of the uncertainty metrics with the number of MC-Dropout passes "
                                             "or ensemble members, from one raw prediction dump: the value of the order "
                                             "as run and the band over random subsets at every count.")
    ap.add_argument("--input_csv", type=str, default="./detailed_results_MCD.csv",
                    help="per-window detail CSV, read for True_Label")
    ap.add_argument("--raw_pred", type=str, default="./mc_raw_pred0205.npy",
                    help="(T, N[, 1]) .npy dump of the passes / members (mc_raw_pred*.npy)")
    ap.add_argument("--balanced_csv", type=str, default=None, help="detail CSV of the balanced set (optional)")
    ap.add_argument("--balanced_raw_pred", type=str, default=None, help="raw dump of the balanced set (optional)")
    ap.add_argument("--counts", type=str, default=None, help="comma-separated counts (default 1,2,3,5,10,15,20,30,...,T)")
    ap.add_argument("--n_orders", type=int, default=100, help="random orders of the passes behind the bands")
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--tolerance", type=float, default=0.05, help="relative distance to the all-T value that counts as converged")
    ap.add_argument("--method", type=str, default="mcd", choices=["mcd", "de"])
    ap.add_argument("--output_dir", type=str, default="./uq_plots/convergence")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..uq import convergence as CV
    from ..uq.drivers import convergence_from_predictions

    def load(csv, raw):
        df = pd.read_csv(csv)
        pred = np.load(raw).astype(np.float32)
        n = pred.shape[1] if pred.ndim >= 2 else pred.shape[0]
        if n != len(df):
            raise ValueError(f"{raw} holds {n} windows, {csv} {len(df)}")
        return CV.on_device(pred), df["True_Label"].to_numpy()

    if bool(a.balanced_csv) != bool(a.balanced_raw_pred):
        raise ValueError("--balanced_csv and --balanced_raw_pred go together")
    counts = [int(c) for c in a.counts.split(",")] if a.counts else None
    label = f"{a.method}_{os.path.splitext(os.path.basename(a.input_csv))[0]}"
    pu, yu = load(a.input_csv, a.raw_pred)
    pb, yb = load(a.balanced_csv, a.balanced_raw_pred) if a.balanced_csv else (None, None)
    res = CV.evaluate_convergence(pu, yu, label, counts=counts, n_orders=a.n_orders, random_state=a.seed,
                                  tolerance=a.tolerance, output_dir=a.output_dir, make_plots=not a.no_plots)
    unit = "passes" if a.method == "mcd" else "members"
    table = pd.DataFrame([{"metric": m, f"{unit}_needed": res[f"passes_needed_{m}"]} for m in CV.METRICS])
    print(f"{pu.shape[0]} {unit}, {pu.shape[1]} windows; tolerance {a.tolerance:g} of the all-{pu.shape[0]} value "
          f"(flip_rate: at most 0.01 of the windows)")
    print(table.to_string(index=False))
    table.to_csv(os.path.join(a.output_dir, f"passes_needed_{label}.csv"), index=False)
    out_csv = os.path.join(a.output_dir, f"convergence_{a.method}.csv")
    convergence_from_predictions(pu, yu, pb, yb, counts, out_csv, n_orders=a.n_orders, seed=a.seed)
    print(f"Saved the curves to: {os.path.join(a.output_dir, f'convergence_{label}.csv')} and {out_csv}")
    return table


def analyze_discrimination(argv=None):
    ap = argparse.ArgumentParser(description="ROC / PR AUC and Mann-Whitney U of a per-window detail CSV with bootstrap CIs: "
                                             "apnea against normal windows (Predicted_Probability) and wrong against "
                                             "right predictions (an uncertainty column).")
    ap.add_argument("--input_csv", type=str, default="./detail_patient_DE.csv")
    ap.add_argument("--score", choices=["Predictive_Entropy", "Predictive_Variance"], default="Predictive_Entropy",
                    help="uncertainty column ranked against 'prediction wrong'")
    ap.add_argument("--cluster", action="store_true", help="resample patients (Patient_ID) instead of windows")
    ap.add_argument("--compare_csv", type=str, default=None,
                    help="detail CSV of a second method over the same windows: paired differences input - compare")
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--no_parity", action="store_true", help="draw with the device counter hash")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots/discrimination")
    ap.add_argument("--output_csv", type=str, default="./discrimination_metrics.csv")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..uq import discrimination as D

    df = pd.read_csv(a.input_csv)
    label = os.path.splitext(os.path.basename(a.input_csv))[0]
    pids = df["Patient_ID"].to_numpy() if a.cluster else None
    y = df["True_Label"].to_numpy()
    common = dict(n_bootstrap=a.n_bootstrap, random_state=a.seed, parity=not a.no_parity, patient_ids=pids)
    res = D.evaluate_discrimination(df["Predicted_Probability"].to_numpy(np.float32), y, label,
                                    score=df[a.score].to_numpy(), output_plot_dir=a.output_plot_dir,
                                    make_plots=not a.no_plots, **common)
    ends = ("_mean", "_ci_lower", "_ci_upper")
    rows = [{"metric": k, "value": v, "mean": res.get(k + "_mean", np.nan), "ci_lower": res.get(k + "_ci_lower", np.nan),
             "ci_upper": res.get(k + "_ci_upper", np.nan)} for k, v in res.items() if not k.endswith(ends)]
    if a.compare_csv:
        other = pd.read_csv(a.compare_csv)
        if len(other) != len(df) or not np.array_equal(other["True_Label"].to_numpy(), y):
            raise ValueError(f"{a.compare_csv} does not hold the windows of {a.input_csv}")
        cmp = D.compare_discrimination(df["Predicted_Probability"].to_numpy(np.float32),
                                       other["Predicted_Probability"].to_numpy(np.float32), y,
                                       score=df[a.score].to_numpy(), score_b=other[a.score].to_numpy(), **common)
        for task in D.TASKS:
            for m in D.METRICS:
                k = f"{task}_{m}"
                rows.append({"metric": k + "_diff", "value": cmp[k + "_diff"], "mean": cmp.get(k + "_diff_mean", np.nan),
                             "ci_lower": cmp.get(k + "_diff_ci_lower", np.nan),
                             "ci_upper": cmp.get(k + "_diff_ci_upper", np.nan)})
                rows.append({"metric": k + "_share_a_gt_b", "value": cmp.get(k + "_share_a_gt_b", np.nan), "mean": np.nan,
                             "ci_lower": np.nan, "ci_upper": np.nan})
    table = pd.DataFrame(rows, columns=["metric", "value", "mean", "ci_lower", "ci_upper"])
    print(f"{'patient-cluster' if a.cluster else 'window'} bootstrap, {a.n_bootstrap} replicates")
    print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
    if a.output_csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.output_csv)), exist_ok=True)
        table.to_csv(a.output_csv, index=False)
    return table


def analyze_recalibration(argv=None):
    ap = argparse.ArgumentParser(description="Temperature / Platt / beta recalibration of a raw prediction dump: fitted "
                                             "on a fit set, or cross-fitted by patient, with ECE / MCE / Brier / NLL "
                                             "before and after on the same bootstrap resamples; writes the calibrated "
                                             "(T, N, 1) dump for the other analyze_* commands.")
    ap.add_argument("--input_csv", type=str, default="./detailed_results_MCD.csv",
                    help="per-window detail CSV, read for True_Label and Patient_ID")
    ap.add_argument("--raw_pred", type=str, default="./mc_raw_pred0205.npy",
                    help="(T, N[, 1]) .npy dump of the passes / members")
    ap.add_argument("--fit_csv", type=str, default=None, help="detail CSV of a separate fit set (optional)")
    ap.add_argument("--fit_raw_pred", type=str, default=None, help="raw dump of the fit set (optional)")
    ap.add_argument("--method", choices=["temperature", "platt", "beta"], default="temperature")
    ap.add_argument("--objective", choices=["joint", "member"], default="joint")
    ap.add_argument("--folds", type=int, default=5, help="patient folds of the cross-fit (without a fit set)")
    ap.add_argument("--n_bins", type=int, default=15)
    ap.add_argument("--n_bootstrap", type=int, default=100)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--no_parity", action="store_true", help="draw with the device counter hash")
    ap.add_argument("--output_raw_pred", type=str, default="./recalibrated_raw_pred.npy")
    ap.add_argument("--output_csv", type=str, default="./recalibration_metrics.csv")
    ap.add_argument("--state", type=str, default=None, help=".npz the fitted map (or the per-fold maps) is saved to")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots/recalibration")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..uq import recalibration as RC

    def load(csv, raw):
        df = pd.read_csv(csv)
        pred = np.load(raw).astype(np.float32)
        n = pred.shape[1] if pred.ndim >= 2 else pred.shape[0]
        if n != len(df):
            raise ValueError(f"{raw} holds {n} windows, {csv} {len(df)}")
        return pred, df

    if bool(a.fit_csv) != bool(a.fit_raw_pred):
        raise ValueError("--fit_csv and --fit_raw_pred go together")
    pred, df = load(a.input_csv, a.raw_pred)
    fit_pred, fit_y = None, None
    if a.fit_csv:
        fit_pred, fit_df = load(a.fit_csv, a.fit_raw_pred)
        fit_y = fit_df["True_Label"].to_numpy()
    label = os.path.splitext(os.path.basename(a.input_csv))[0]
    pids = df["Patient_ID"].to_numpy() if "Patient_ID" in df.columns else None
    res, det = RC.evaluate_recalibration(pred, df["True_Label"].to_numpy(), label, fit_predictions=fit_pred, fit_y=fit_y,
                                         patient_ids=pids, n_folds=a.folds, method=a.method, objective=a.objective,
                                         n_bootstrap=a.n_bootstrap, random_state=a.seed, parity=not a.no_parity,
                                         n_bins=a.n_bins, output_plot_dir=a.output_plot_dir, make_plots=not a.no_plots,
                                         seed=a.seed, return_details=True)
    cols = ["before", "after", "diff", "diff_mean", "diff_ci_lower", "diff_ci_upper", "share_improved"]
    table = pd.DataFrame([{"metric": m, **{c: res.get(f"{m}_{c}", np.nan) for c in cols}} for m in RC.METRICS],
                         columns=["metric"] + cols)
    print(f"{a.method} / {a.objective}, " + ("fitted on the fit set" if a.fit_csv else f"cross-fitted in {a.folds} folds"))
    print({k: v for k, v in res.items() if k.startswith(("theta", "temperature", "fit_nll", "converged", "n_iter"))})
    print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
    for path in (a.output_csv, a.output_raw_pred, a.state):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if a.output_csv:
        table.to_csv(a.output_csv, index=False)
    if a.output_raw_pred:
        np.save(a.output_raw_pred, np.asarray(det["calibrated"], np.float32))
        print(f"Saved the calibrated predictions to: {a.output_raw_pred}")
    if a.state:
        if a.fit_csv:
            det["fit"].save(a.state)
        else:
            info = det["fit"]
            np.savez(a.state, theta=info["theta"], fold=info["fold"],
                     meta=np.array(json.dumps({"method": a.method, "objective": a.objective, "seed": a.seed,
                                               "converged": info["converged"], "n_iter": info["n_iter"]})))
    return table


def analyze_conformal(argv=None):
    ap = argparse.ArgumentParser(description="Split conformal prediction sets from a per-window detail CSV: with a fit "
                                             "CSV the thresholds are calibrated there and the set code of every input "
                                             "window is written; without one, coverage and set sizes over random "
                                             "calibration / test splits of the patients.")
    ap.add_argument("--input_csv", type=str, default="./detail_patient_DE.csv",
                    help="per-window detail CSV, read for Predicted_Probability, True_Label and Patient_ID")
    ap.add_argument("--fit_csv", type=str, default=None, help="detail CSV of a separate calibration set (optional)")
    ap.add_argument("--alphas", type=str, default="0.01,0.025,0.05,0.1,0.15,0.2", help="comma-separated miscoverage levels")
    ap.add_argument("--n_splits", type=int, default=1000)
    ap.add_argument("--cal_fraction", type=float, default=0.5)
    ap.add_argument("--cluster", choices=["pooled", "subsample"], default="pooled")
    ap.add_argument("--mode", choices=["class_conditional", "marginal"], default="class_conditional")
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--output_csv", type=str, default="./conformal_metrics.csv")
    ap.add_argument("--state", type=str, default=None, help=".npz the fitted thresholds are saved to (with --fit_csv)")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots/conformal")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..ops import conformal as conf_ops
    from ..uq import conformal as CF

    df = pd.read_csv(a.input_csv)
    alphas = [float(v) for v in a.alphas.split(",") if v.strip()]
    sufs = CF.level_suffixes(alphas)
    p = df["Predicted_Probability"].to_numpy(np.float32)
    has_y = "True_Label" in df.columns
    for path in (a.output_csv, a.state):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if a.fit_csv:
        fit = pd.read_csv(a.fit_csv)
        rows = []
        for alpha, suf in zip(alphas, sufs):
            cp = CF.conformal_calibrate(fit["Predicted_Probability"].to_numpy(np.float32), fit["True_Label"].to_numpy(),
                                        alpha, a.mode)
            sets = cp.predict_sets(p)
            df[f"Conformal_Set{suf}"] = sets
            if a.state:
                stem = a.state[:-4] if a.state.endswith(".npz") else a.state
                cp.save(stem + (suf if len(alphas) > 1 else ""))
            row = {"alpha": alpha, "tau0": cp.tau0, "tau1": cp.tau1, "qhat": cp.qhat}
            if has_y:
                row.update(CF.conformal_metrics(sets, df["True_Label"].to_numpy(), valid=np.isfinite(p)))
            rows.append(row)
        table = pd.DataFrame(rows)
        print(f"{a.mode}: thresholds calibrated on {len(fit)} windows of {a.fit_csv}")
        print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
        if a.output_csv:
            df.to_csv(a.output_csv, index=False)
            print(f"Saved the set codes (bit 0 = normal, bit 1 = apnea) to: {a.output_csv}")
        return table
    label = os.path.splitext(os.path.basename(a.input_csv))[0]
    pids = df["Patient_ID"].to_numpy() if "Patient_ID" in df.columns else None
    res = CF.evaluate_conformal(p, df["True_Label"].to_numpy(), label, alphas=alphas, n_splits=a.n_splits,
                                cal_fraction=a.cal_fraction, patient_ids=pids, cluster=a.cluster, mode=a.mode,
                                random_state=a.seed, output_dir=a.output_plot_dir, make_plots=not a.no_plots)
    rows = [{"metric": m, "alpha": alpha, "mean": res[f"{m}{suf}"], "ci_lower": res[f"{m}{suf}_ci_lower"],
             "ci_upper": res[f"{m}{suf}_ci_upper"]} for alpha, suf in zip(alphas, sufs) for m in conf_ops.METRICS]
    rows += [{"metric": "coverage_violation_rate", "alpha": alpha, "mean": res[f"coverage_violation_rate{suf}"],
              "ci_lower": np.nan, "ci_upper": np.nan} for alpha, suf in zip(alphas, sufs)]
    table = pd.DataFrame(rows, columns=["metric", "alpha", "mean", "ci_lower", "ci_upper"])
    print(f"{a.mode} / {a.cluster}: {a.n_splits} splits of {res['n_units']} "
          f"{'patients' if pids is not None else 'windows'}, {res['n_valid']} valid windows")
    print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
    if a.output_csv:
        table.to_csv(a.output_csv, index=False)
    return table


def analyze_shift_robustness(argv=None):
    ap = argparse.ArgumentParser(description="Uncertainty under signal corruption: one sampler on degraded, "
                                             "re-standardised copies of the unbalanced test windows; one row per "
                                             "(corruption, severity) plus the clean row.")
    _uq_common(ap)
    ap.add_argument("--method", choices=["mcd", "de", "laplace"], default="mcd")
    ap.add_argument("--model_path", type=str, default="./AlCNN1D_no_pool.keras")
    ap.add_argument("--n_passes", type=int, default=50, help="MC Dropout passes / Laplace samples")
    ap.add_argument("--bn_mode", choices=["batch", "running"], default="batch",
                    help="batch = reference semantics: the BatchNorm statistics are those of the corrupted set")
    ap.add_argument("--model_dir", type=str, default="./models/ensemble_cnn_no_pool", help="--method de")
    ap.add_argument("--pattern", type=str, default="AlCNN_smote_seed{}.keras")
    ap.add_argument("--num_members", type=int, default=5)
    ap.add_argument("--offset", type=int, default=5, help="file index of member 0 (reference loader uses i+5)")
    ap.add_argument("--kinds", type=str, default="all", help="comma-separated corruption kinds, or 'all'")
    ap.add_argument("--severities", type=str, default="1,2,3,4,5")
    ap.add_argument("--channels", type=str, default="all", help="comma-separated channel indices, or 'all'")
    ap.add_argument("--state", type=str, default="./laplace_state.npz", help="--method laplace: the fitted posterior")
    ap.add_argument("--conformal_state", type=str, default="",
                    help="a ConformalPredictor .npz calibrated on clean data: adds coverage and set shares")
    ap.add_argument("--output_plot_dir", type=str, default="./uq_plots_patient/shift_robustness")
    ap.add_argument("--output_csv", type=str, default="./uq_results_shift/shift_robustness.csv")
    a = ap.parse_args(argv)
    from ..models.cnn import load_model
    from ..uq import robustness as RB

    np.random.seed(a.seed)
    Xu, yu, pids, _, _ = _load_test(a.data_dir)
    if a.method == "de":
        from ..parallel.ensemble import load_ensemble

        predict = RB.deep_ensemble_predictor(load_ensemble(a.model_dir, a.pattern, a.num_members, a.offset))
    elif a.method == "laplace":
        from ..uq.laplace import LaplaceState

        predict = RB.laplace_predictor(load_model(a.model_path), LaplaceState.load(a.state), a.n_passes, a.seed)
    else:
        predict = RB.mc_dropout_predictor(load_model(a.model_path), a.n_passes, a.bn_mode, a.seed)
    conformal = None
    if a.conformal_state:
        from ..uq.conformal import ConformalPredictor

        conformal = ConformalPredictor.load(a.conformal_state)
    kinds = RB.KINDS if a.kinds == "all" else tuple(k.strip() for k in a.kinds.split(","))
    channels = None if a.channels == "all" else [int(c) for c in a.channels.split(",")]
    conds = RB.shift_conditions(kinds, [int(s) for s in a.severities.split(",")], channels)
    table = RB.evaluate_shift(predict, Xu, yu, conds, seed=a.seed, patient_ids=pids, conformal=conformal,
                              n_bootstrap=a.n_bootstrap)
    d = os.path.dirname(a.output_csv)
    if d:
        os.makedirs(d, exist_ok=True)
    table.to_csv(a.output_csv, index=False)
    print(f"Saved the shift table ({len(table)} rows) to {a.output_csv}")
    if not a.no_plots:
        RB.plot_shift({a.method: table}, a.output_plot_dir)
    return table


def analyze_ensemble_members(argv=None):
    ap = argparse.ArgumentParser(description="Ensemble composition from one raw prediction dump: every member alone and "
                                             "by what the ensemble loses without it, the pairwise diversity, and greedy "
                                             "pruning (selected on some patients, scored on the others) against the "
                                             "first k and random k members; writes the pruned (k, N, 1) dump for the "
                                             "other analyze_* commands.")
    ap.add_argument("--input_csv", type=str, default="./detail_patient_DE.csv",
                    help="per-window detail CSV, read for True_Label and Patient_ID")
    ap.add_argument("--raw_pred", type=str, default="./de_raw_pred.npy", help="(T, N[, 1]) .npy dump of the members")
    ap.add_argument("--loss", choices=["nll", "brier"], default="nll", help="the loss the saved selection minimises")
    ap.add_argument("--folds", type=int, default=5, help="patient folds of the cross-fit (1: none)")
    ap.add_argument("--k_max", type=int, default=None, help="length of the saved selection path (default T)")
    ap.add_argument("--replacement", action="store_true", help="the saved selection may pick a member again")
    ap.add_argument("--n_orders", type=int, default=100, help="random orders of the members behind the bands")
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--tolerance", type=float, default=None,
                    help="absolute distance to the all-T loss that counts as enough (default 0.001)")
    ap.add_argument("--output_csv", type=str, default="./ensemble_members.csv")
    ap.add_argument("--state", type=str, default=None, help=".npz the selection is saved to")
    ap.add_argument("--output_raw_pred", type=str, default=None, help="pruned (keep, N, 1) dump (with --keep)")
    ap.add_argument("--keep", type=int, default=None, help="members of the pruned dump")
    ap.add_argument("--output_dir", type=str, default="./uq_plots/members")
    ap.add_argument("--no_plots", action="store_true")
    a = ap.parse_args(argv)
    import pandas as pd

    from ..uq import members as MM

    if bool(a.output_raw_pred) != (a.keep is not None):
        raise ValueError("--output_raw_pred and --keep go together")
    df = pd.read_csv(a.input_csv)
    pred = np.load(a.raw_pred).astype(np.float32)
    n = pred.shape[1] if pred.ndim >= 2 else pred.shape[0]
    if n != len(df):
        raise ValueError(f"{a.raw_pred} holds {n} windows, {a.input_csv} {len(df)}")
    y = df["True_Label"].to_numpy()
    pids = df["Patient_ID"].to_numpy() if "Patient_ID" in df.columns else None
    label = os.path.splitext(os.path.basename(a.input_csv))[0]
    dev = MM.on_device(pred)
    tol = MM.DEFAULT_TOLERANCE if a.tolerance is None else a.tolerance
    res, det = MM.evaluate_members(dev, y, label, patient_ids=pids, n_folds=a.folds, n_orders=a.n_orders, tolerance=tol,
                                   random_state=a.seed, output_dir=a.output_dir, make_plots=not a.no_plots,
                                   return_details=True)
    tab = det["table"]
    t_count = dev.shape[0]
    cols = ("accuracy", "sensitivity", "specificity", "nll", "brier", "loo_nll_delta", "loo_brier_delta")
    table = pd.DataFrame({"member": np.arange(t_count), **{k: np.resize(tab[k], t_count) for k in cols}})
    print(f"{t_count} members, {tab['n_valid']} valid windows; ensemble NLL {res['ensemble_nll']:.6f}, Brier "
          f"{res['ensemble_brier']:.6f}; mean disagreement {res['mean_disagreement']:.6f}, ambiguity {res['ambiguity']:.6f}")
    print(table.to_string(index=False, float_format=lambda v: f"{v:.6f}"))
    print(f"members_needed_nll = {res['members_needed_nll']}, members_needed_brier = {res['members_needed_brier']} "
          f"(greedy, {'held out over ' + str(a.folds) + ' patient folds' if a.folds > 1 else 'on the selection windows'}, "
          f"within {tol:g} of all {t_count})")
    for path in (a.output_csv, a.state, a.output_raw_pred):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if a.output_csv:
        table.to_csv(a.output_csv, index=False)
    if a.state or a.output_raw_pred:
        sel = det["selection"][a.loss]   # the whole path without replacement is what evaluate_members selected
        if a.replacement or a.k_max is not None:
            sel = MM.select_members(dev, y, loss=a.loss, k_max=a.k_max, replacement=a.replacement, groups=pids,
                                    n_folds=a.folds if t_count > 1 else 1, seed=a.seed)
        if a.state:
            sel.save(a.state)
        if a.output_raw_pred:
            np.save(a.output_raw_pred, np.asarray(sel.apply(pred, a.keep), np.float32))
            print(f"Saved the {a.keep} members {sel.order[:a.keep].tolist()} to: {a.output_raw_pred}")
    return table


def uq_demo(argv=None):
    ap = argparse.ArgumentParser(description="Synthetic UQ evaluation demo (uq_techniques.py __main__).")
    ap.add_argument("--output_plot_dir", default="./dummy_uq_plots")
    a = ap.parse_args(argv)
    from ..uq.uq_techniques import demo

    return demo(a.output_plot_dir)


COMMANDS = {name: fn for name, fn in globals().items()
            if callable(fn) and not name.startswith("_") and name not in ("main",) and fn.__module__ == __name__}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help") or argv[0] not in COMMANDS:
        print("usage: python -m uncertaintyquantification_sleepapnea_1dcnn_amd <command> [flags]\ncommands:\n  " +
              "\n  ".join(sorted(COMMANDS)))
        return 0 if (argv and argv[0] in ("-h", "--help")) else (2 if argv else 0)
    COMMANDS[argv[0]](argv[1:])
    return 0
