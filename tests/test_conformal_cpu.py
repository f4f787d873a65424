"""Conformal prediction on the CPU: the rank formula, the torch emulation against the literal golden, the public
API composed by hand against ``evaluate_conformal``, and the finite-sample validity theorem."""
import os
import warnings

import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import conformal as ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import conformal as CF

from . import conformal_fixtures as F
from .patient_fixtures import cohort


def evaluate(*args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=UserWarning)
        return CF.evaluate_conformal(*args, make_plots=False, return_details=True, **kw)


def test_rank_formula():
    """k(n) = ceil((n + 1)(1 - alpha)) in integers, with the exact products and k > n."""
    want = {100_000: {8: 9, 9: 9, 10: 10, 19: 18, 99: 90},    # (9 + 1) 0.9 = 9, (19 + 1) 0.9 = 18, 100 0.9 = 90: exact
            50_000: {8: 9, 9: 10, 10: 11, 19: 19, 99: 95}}    # (19 + 1) 0.95 = 19 exactly
    for ppm, row in want.items():
        for n, k in row.items():
            assert int(ops.rank_k(n, ppm)) == k
            assert int(ops.rank_k(torch.tensor(n), torch.tensor(ppm))) == k
            assert int(ops.rank_k(np.int64(n), np.int64(ppm))) == k
    assert ops.rank_k(8, 100_000) > 8 and ops.rank_k(9, 50_000) > 9 and ops.rank_k(0, 500_000) == 1   # k > n
    assert ops.alpha_to_ppm([0.1, 0.025, 1e-6]).tolist() == [100_000, 25_000, 1]
    for bad in ([0.0], [1.0], [-0.1], [np.nan], [], [4e-7]):
        with pytest.raises(ValueError):
            ops.alpha_to_ppm(bad)
    assert ops.cal_threshold(0) == 0 and ops.cal_threshold(0.5) == 1 << 31 and ops.cal_threshold(1) == 1 << 32
    with pytest.raises(ValueError):
        ops.cal_threshold(1.5)


def test_split_hash_is_the_documented_function():
    """ops/rng.py split_hash on tensors against the scalar definition: boot_key under a salt, then mix(key ^ mix(u))."""
    for seed, r, u, salt in ((0, 0, 0, rng.SPLIT_SALT), (2025, 7, 123456, rng.SPLIT_SALT), (0xFFFFFFFF, 999, 2 ** 31 - 1,
                                                                                            rng.SPLIT_SALT2)):
        key = rng.mix32_int((seed ^ salt) ^ rng.mix32_int((r * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF))
        want = rng.mix32_int(key ^ rng.mix32_int(u))
        assert int(rng.split_hash(seed, r, torch.tensor(u), salt)) == want
    u = torch.arange(200_000)
    share = float((rng.split_hash(3, 1, u) < (1 << 32) // 4).double().mean())
    assert abs(share - 0.25) < 5 * np.sqrt(0.25 * 0.75 / 200_000)
    assert not torch.equal(rng.split_hash(3, 1, u), rng.split_hash2(3, 1, u))
    assert not torch.equal(rng.split_hash(3, 1, u), rng.split_hash(3, 2, u))


@pytest.mark.parametrize("mode", CF.MODES)
@pytest.mark.parametrize("structure", F.STRUCTURES)
@pytest.mark.parametrize("n", [1, 2, 70, 257, 3001])
def test_emulation_matches_golden(n, structure, mode):
    p, y = F.make_case(n, structure)
    for cluster in CF.CLUSTERS:
        F.check_against_golden(p, y, F.make_ids(n, "few"), cluster, mode, n_splits=3 if n < 3001 else 2)


@pytest.mark.parametrize("mode", CF.MODES)
@pytest.mark.parametrize("cluster", CF.CLUSTERS)
@pytest.mark.parametrize("units", F.UNITS)
def test_units_and_calibration_fractions(units, cluster, mode):
    p, y = F.make_case(257, "levels8")
    for cal_fraction in (0.0, 0.5, 1.0):
        totals, counts = F.check_against_golden(p, y, F.make_ids(257, units), cluster, mode, cal_fraction, n_splits=4)
        if cal_fraction == 0.0:     # nothing calibrates: infinite thresholds, every window gets both labels
            assert int(totals[:, :2].sum()) == 0
            assert torch.equal(counts[..., ops.COLS.index("both_0")], counts[..., ops.COLS.index("n_test_0")])
        if cal_fraction == 1.0:
            assert int(totals[:, 2:].sum()) == 0 and int(counts.sum()) == 0
    if units == "one" and cluster == "subsample":   # one patient: at most one calibration window
        assert int(totals[:, :2].sum(1).max()) <= 1


@pytest.mark.parametrize("mode", CF.MODES)
def test_single_class_and_nan_means(mode):
    p, y = F.make_case(257, "continuous")
    ids = F.make_ids(257, "few")
    for cluster in CF.CLUSTERS:
        for yy in (np.zeros_like(y), np.ones_like(y)):
            F.check_against_golden(p, yy, ids, cluster, mode)
        q = p.copy()
        q[[0, 5, 100, 256]] = [np.nan, np.inf, -np.inf, np.nan]
        F.check_against_golden(q, y, ids, cluster, mode)
    F.check_against_golden(np.full(20, np.nan, np.float32), y[:20], None, "pooled", mode)
    F.check_against_golden(p, y, ids, "pooled", mode, r0=5, n_splits=2)


def test_later_chunk_and_sort_invariants():
    p, y = F.make_case(513, "levels8")
    ids = F.make_ids(513, "few")
    pp = F.prepare(p, y, ids, "subsample", "class_conditional")
    ppm = torch.as_tensor(ops.alpha_to_ppm(F.ALPHAS), dtype=torch.int32)
    full = CF._split_counts(pp, 3, 0, 8, 1 << 31, ppm, "class_conditional")
    part = CF._split_counts(pp, 3, 3, 4, 1 << 31, ppm, "class_conditional")
    assert torch.equal(part[0], full[0][3:7]) and torch.equal(part[1], full[1][3:7])
    gs, ge = ops.group_bounds(torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.bool))
    assert gs.tolist() == [0, 0, 0, 3, 4, 4] and ge.tolist() == [3, 3, 3, 4, 6, 6]
    # class-conditional sets do not change under a strictly increasing map of p; marginal sets may
    a = evaluate(p, y, "a", n_splits=5, patient_ids=ids)[1]
    b = evaluate((p.astype(np.float64) ** 3).astype(np.float32) / 2, y, "b", n_splits=5, patient_ids=ids)[1]
    np.testing.assert_array_equal(a["counts"], b["counts"])


@pytest.mark.parametrize("mode", CF.MODES)
@pytest.mark.parametrize("cluster", CF.CLUSTERS)
def test_composition_equals_evaluate(mode, cluster):
    """calibrate on a split's calibration windows, predict its test windows, score them: the row of evaluate_conformal."""
    p, y = F.make_case(700, "levels8" if mode == "marginal" else "continuous")
    p[3] = np.nan
    ids = F.make_ids(700, "few")
    alphas = (0.05, 0.2)
    res, det = evaluate(p, y, "c", alphas=alphas, n_splits=6, cal_fraction=0.4, patient_ids=ids, cluster=cluster,
                        mode=mode, random_state=11)
    assert res["n_valid"] == 699 and res["n_splits"] == 6 and res["n_units"] == len(np.unique(ids))
    for r in (0, 2, 5):
        cal, test = CF.split_masks(p, 11, r, 0.4, ids, cluster)
        assert not (cal & test).any() and not cal[3] and not test[3]
        for j, alpha in enumerate(alphas):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", category=RuntimeWarning)
                cp = CF.conformal_calibrate(p[cal], y[cal], alpha, mode)
            got = CF.conformal_metrics(cp.predict_sets(p[test]), y[test])
            for m in ops.METRICS:
                np.testing.assert_equal(got[m], float(det[m][r, j]), err_msg=m)
            assert got["n_valid"] == int(det["n_valid"][r, j]) == int(test.sum())
            g = CF.golden_conformal_split(p, y, cal, test, int(det["alpha_ppm"][j]), mode)
            np.testing.assert_array_equal(cp.predict_sets(p), g["sets"])
            assert cp.k == g["k"] and cp.n_cal == g["n_cal"]
    for m in ops.METRICS:
        mean, lo, hi = C._ci(det[m][:, 1])
        assert (res[f"{m}_at_0.20"], res[f"{m}_at_0.20_ci_lower"], res[f"{m}_at_0.20_ci_upper"]) == (mean, lo, hi)
    cov, n = det["counts"][..., [1, 7]].sum(-1), det["n_valid"]
    assert res["coverage_violation_rate_at_0.05"] == float(np.mean(cov[:, 0] * 20 < n[:, 0] * 19))


@pytest.fixture(scope="module")
def validity():
    """R = 2000 window splits of the synthetic cohort at three levels, computed once."""
    probs, y, _ = cohort(4)
    p = probs.mean(0, dtype=np.float32)
    assert len(np.unique(p[y == 0])) == int((y == 0).sum()) and len(np.unique(p[y == 1])) == int((y == 1).sum())
    return evaluate(p, y, "validity", alphas=(0.05, 0.1, 0.2), n_splits=2000, random_state=2025)[1]


@pytest.mark.parametrize("z", [0, 1])
@pytest.mark.parametrize("j", [0, 1, 2])
def test_finite_sample_validity(validity, j, z):
    """Theory, not the code against itself: with window units and distinct scores the test coverage of class z has
    expectation k / (n_cal,z + 1) given n_cal,z (a test window's rank among the calibration windows and itself is
    uniform).  |mean_r coverage_z - mean_r k_z / (n_cal,z(r) + 1)| <= 4 sd_r / sqrt(R)."""
    det = validity
    cov = det[f"coverage_class_{z}"][:, j]
    n_cal = det["totals"][:, z]
    k = ops.rank_k(n_cal, int(det["alpha_ppm"][j]))
    assert np.all(k <= n_cal) and not np.isnan(cov).any()
    expect = k / (n_cal + 1.0)
    gap, bound = abs(cov.mean() - expect.mean()), 4 * cov.std(ddof=1) / np.sqrt(len(cov))
    print(f"class {z}, alpha {det['alpha_ppm'][j] / 1e6}: coverage {cov.mean():.5f}, theory {expect.mean():.5f}, "
          f"gap {gap:.2e}, bound {bound:.2e}")
    assert gap <= bound


def test_predictor_save_load_and_infinite_thresholds(tmp_path):
    p, y = F.make_case(300, "continuous")
    for mode in CF.MODES:
        cp = CF.conformal_calibrate(p, y, 0.1, mode)
        back = CF.ConformalPredictor.load(cp.save(str(tmp_path / f"cp_{mode}")))
        assert back == cp and back.alpha == 0.1
        np.testing.assert_array_equal(back.predict_sets(p), cp.predict_sets(p))
        sets = cp.predict_sets(torch.from_numpy(p))
        assert isinstance(sets, torch.Tensor) and sets.dtype == torch.uint8 and tuple(sets.shape) == (300,)
        m = CF.conformal_metrics(cp.predict_sets(p), y)
        assert m["coverage"] >= 0.9 and m["n_valid"] == 300   # the calibration set itself: at least k / n
        assert abs(m["share_empty"] + m["share_singleton"] + m["share_both"] - 1) < 1e-12
    assert sorted(np.load(tmp_path / "cp_marginal.npz", allow_pickle=False).files) == ["meta", "thresholds"]
    # a class without calibration windows: an infinite threshold and one warning
    with pytest.warns(RuntimeWarning) as rec:
        cp = CF.conformal_calibrate(p, np.zeros_like(y), 0.1)
    assert len(rec) == 1 and cp.tau1 == -np.inf and cp.n_cal == (300, 0) and np.isfinite(cp.tau0)
    assert bool(np.all(cp.predict_sets(p) & 2))
    assert CF.ConformalPredictor.load(cp.save(str(tmp_path / "inf.npz"))) == cp
    # too few windows for the level: k > n, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cp = CF.conformal_calibrate(p[:12], y[:12], 0.01)
    assert cp.tau0 == np.inf and cp.tau1 == -np.inf and bool(np.all(cp.predict_sets(p) == 3))
    q = p.copy()
    q[7] = np.nan
    assert CF.conformal_calibrate(p, y, 0.2).predict_sets(q)[7] == 3
    assert CF.conformal_metrics([3, 0, 1, 2], [0, 1, 1, 1], valid=[True, True, True, False]) == {
        "coverage": 1 / 3, "coverage_class_0": 1.0, "coverage_class_1": 0.0, "share_empty": 1 / 3,
        "share_singleton": 1 / 3, "share_both": 1 / 3, "mean_set_size": 1.0, "singleton_accuracy": 0.0, "n_valid": 3}


def test_argument_errors():
    p, y = F.make_case(50, "continuous")
    for kw in (dict(mode="adaptive"), dict(cluster="bootstrap"), dict(alphas=(0.0, 0.1)), dict(alphas=()),
               dict(alphas=np.linspace(0.01, 0.9, 33)), dict(n_splits=0), dict(cal_fraction=1.5),
               dict(patient_ids=np.arange(49))):
        with pytest.raises(ValueError):
            evaluate(p, y, "e", **kw)
    with pytest.raises(ValueError):
        evaluate(p, y[:-1], "e")
    with pytest.raises(ValueError):
        evaluate(p, y + 1, "e")
    with pytest.raises(ValueError):
        CF.conformal_calibrate(p, y, (0.1, 0.2))
    with pytest.raises(ValueError):
        CF.conformal_calibrate(p, y[:-1])
    with pytest.raises(ValueError):
        CF.conformal_calibrate(p, y, mode="mondrian")
    with pytest.raises(ValueError):
        CF.conformal_metrics([4], [0])
    with pytest.raises(ValueError):
        CF.conformal_metrics([1, 2], [0])
    unit, packed = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8)
    ppm = torch.tensor([100_000], dtype=torch.int32)
    for bad in (dict(unit=unit.long()), dict(packed=packed[:3]), dict(within=unit), dict(cal_thr=-1), dict(r0=-1),
                dict(strata=3), dict(ppm=torch.ones(33, dtype=torch.int32))):
        kw = dict(unit=unit, packed=packed, within=None, ucount=None, cal_thr=1 << 31, r0=0, strata=2, ppm=ppm)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.select_eager(kw["unit"], kw["packed"], kw["within"], kw["ucount"], 0, kw["r0"], 2, kw["cal_thr"],
                             kw["ppm"], kw["strata"])
    with pytest.raises(ValueError):
        ops.count_eager(unit, packed, None, None, 0, 0, 1 << 31, torch.zeros(2, 65, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.finalize(np.zeros((2, 9)))
    with pytest.warns(UserWarning, match="patient_ids"):
        CF.evaluate_conformal(p, y, "w", n_splits=2, make_plots=False)


def test_plots_keys_and_reexports(tmp_path):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import uq_techniques as UT

    p, y = F.make_case(400, "continuous")
    res = CF.evaluate_conformal(p[None, :, None], y, "fixture", n_splits=20, patient_ids=F.make_ids(400, "few"),
                                output_dir=str(tmp_path))
    for suf in ("_at_0.010", "_at_0.025", "_at_0.050", "_at_0.100", "_at_0.150", "_at_0.200"):
        for m in ops.METRICS:
            assert {f"{m}{suf}", f"{m}{suf}_ci_lower", f"{m}{suf}_ci_upper"} <= set(res)
        assert 0.0 <= res[f"coverage_violation_rate{suf}"] <= 1.0
        assert res[f"coverage{suf}_ci_lower"] <= res[f"coverage{suf}"] <= res[f"coverage{suf}_ci_upper"]
    assert C.plt is None or (os.path.exists(tmp_path / "conformal_coverage_fixture.png") and
                             os.path.exists(tmp_path / "conformal_set_types_fixture.png"))
    assert UT.evaluate_conformal is CF.evaluate_conformal and UT.conformal_calibrate is CF.conformal_calibrate
    assert UT.conformal_metrics is CF.conformal_metrics and UT.ConformalPredictor is CF.ConformalPredictor
    assert UT.golden_conformal_split is CF.golden_conformal_split


def test_cli_both_forms(tmp_path):
    import pandas as pd

    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli.commands import COMMANDS

    p, y = F.make_case(600, "continuous")
    ids = F.make_ids(600, "few")
    csv, fit_csv = tmp_path / "detail.csv", tmp_path / "fit.csv"
    frame = pd.DataFrame({"Patient_ID": ids, "True_Label": y, "Predicted_Probability": p})
    frame.iloc[:350].to_csv(csv, index=False)
    frame.iloc[350:].to_csv(fit_csv, index=False)
    p_in, y_in, p_fit, y_fit = (pd.read_csv(csv)["Predicted_Probability"].to_numpy(np.float32), y[:350],
                                pd.read_csv(fit_csv)["Predicted_Probability"].to_numpy(np.float32), y[350:])
    out, state = tmp_path / "out" / "m.csv", tmp_path / "state.npz"
    table = COMMANDS["analyze_conformal"]([
        "--input_csv", str(csv), "--alphas", "0.05,0.2", "--n_splits", "30", "--cal_fraction", "0.4", "--cluster",
        "subsample", "--mode", "marginal", "--seed", "3", "--output_csv", str(out), "--no_plots"])
    want = evaluate(p_in, y_in, "x", alphas=(0.05, 0.2), n_splits=30, cal_fraction=0.4, patient_ids=ids[:350],
                    cluster="subsample", mode="marginal", random_state=3)[0]
    saved = pd.read_csv(out)
    assert list(saved["metric"]) == list(table["metric"]) and len(saved) == 2 * (len(ops.METRICS) + 1)
    row = saved[(saved["metric"] == "coverage") & (saved["alpha"] == 0.2)].iloc[0]
    assert abs(row["mean"] - want["coverage_at_0.20"]) < 1e-12 and abs(row["ci_upper"] - want["coverage_at_0.20_ci_upper"]) < 1e-12
    # with a fit CSV: thresholds from there, a set code per input window, a state that loads back
    table = COMMANDS["analyze_conformal"]([
        "--input_csv", str(csv), "--fit_csv", str(fit_csv), "--alphas", "0.1", "--output_csv", str(out), "--state",
        str(state)])
    cp = CF.ConformalPredictor.load(str(state))
    assert cp == CF.conformal_calibrate(p_fit, y_fit, 0.1)
    sets = pd.read_csv(out)["Conformal_Set_at_0.10"].to_numpy()
    np.testing.assert_array_equal(sets, cp.predict_sets(p_in))
    assert abs(table["coverage"][0] - CF.conformal_metrics(sets, y_in)["coverage"]) < 1e-15
