"""Recalibration on the CPU: the torch emulation and the Newton fit against the float64 goldens, the public API."""
import os

import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import calib, recal
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import recalibration as RC
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import uq_techniques as UT

from . import recalibration_fixtures as F
from .dist_utils import run_ranks

U = 2.0 ** -52


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _eager(p, y, fold, th, nf, obj, **kw):
    return recal.sums_eager(_t(p), _t(y), None if fold is None else _t(fold), _t(th), nf, obj, **kw)


def allowance(out, absum, T):
    """``(n_valid + T + 16) 2^-52 abs_sum``: ordered summation of n_valid terms, T inner terms and a few ulps of
    exp / log / division per term."""
    return (out[..., :1] + T + 16) * U * absum


@pytest.mark.parametrize("objective", RC.OBJECTIVES)
@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("T,n,nf,layout", [(1, 65, 1, "grouped"), (3, 257, 5, "grouped"), (7, 300, 4, "shuffled")])
def test_emulation_matches_golden(T, n, nf, layout, kind, objective):
    p, y = F.variant(n, T, kind)
    fold = F.fold_codes(n, nf, layout) if nf > 1 else None
    th = F.candidates(5)
    ref = RC.golden_sums(p, y, fold, th, nf, objective)
    got, ab = (v.numpy() for v in _eager(p, y, fold, th, nf, objective, return_abs=True))
    assert got.shape == (nf, 5, 12)
    np.testing.assert_array_equal(got[..., :2], ref[..., :2])
    bad = int(kind in ("nan", "label2")) + int(kind == "nan" and n > 4) + (2 if nf > 1 else 0)
    assert got[:, 0, 0].sum() == n - bad
    ratio = np.abs(got - ref)[..., 2:] / np.maximum(allowance(got, ab, T)[..., 2:], 1e-300)
    print(f"T={T} n={n} F={nf} {kind} {objective}: max deviation / allowance {ratio.max():.3f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("objective", RC.OBJECTIVES)
def test_gradient_and_hessian_match_central_differences(objective):
    p, y = F.ensemble(257, 3, seed=5)
    th0 = np.array([0.7, 0.5, -0.2])
    h = 1e-5

    def row(th):
        return _eager(p, y, None, np.asarray(th, np.float64)[None], 1, objective).numpy()[0, 0]

    loss, g, H = RC.unpack_sums(row(th0))
    gn, Hn = np.zeros(3), np.zeros((3, 3))
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        rp, rm = row(th0 + e), row(th0 - e)
        gn[i] = (rp[2] - rm[2]) / (2 * h)
        Hn[i] = (RC.unpack_sums(rp)[1] - RC.unpack_sums(rm)[1]) / (2 * h)
    assert np.max(np.abs(g - gn)) <= 1e-6 * np.max(np.abs(g))
    assert np.max(np.abs(H - Hn)) <= 1e-6 * np.max(np.abs(H))


@pytest.mark.parametrize("objective", RC.OBJECTIVES)
@pytest.mark.parametrize("method", RC.METHODS)
def test_fit_matches_golden(method, objective):
    p, y, _ = F.fit_set()
    g = F.golden_facts(method, objective)
    r = RC.fit_recalibration(p, y, method, objective)
    assert r.converged and r.constrained == () and r.n_valid == g["n_valid"] == F.FIT_N
    assert r.n_iter <= 10 and r.grad_norm <= 1e-8
    assert np.max(np.abs(r.theta - g["theta"])) <= F.theta_bound(g)
    assert abs(r.nll_after - g["nll"]) <= 1e-12
    assert r.nll_after < r.nll_before
    assert (r.temperature is not None) == (method == "temperature")
    if method == "temperature":
        assert r.theta[0] == r.theta[1] and r.theta[2] == 0.0 and abs(r.temperature - 1.0 / r.theta[0]) < 1e-15
    if method == "platt":
        assert r.theta[0] == r.theta[1]


def test_identity_loss_is_the_calibration_nll():
    p, y = F.ensemble(500, 1, seed=8)
    p[0, 0], p[0, 1] = 0.0, 1.0
    r = RC.fit_recalibration(p, y, "temperature")
    assert abs(r.nll_before - C.golden_calibration(p[0].astype(np.float64), y)["nll"]) <= 1e-12


def test_platt_member_single_pass_is_logistic_regression():
    from sklearn.linear_model import LogisticRegression

    p, y = F.ensemble(800, 1, seed=9)
    r = RC.fit_recalibration(p, y, "platt", "member")
    pc = np.clip(p[0].astype(np.float64), 1e-7, 1 - 1e-7)
    x = (np.log(pc) - np.log1p(-pc))[:, None]
    lr = LogisticRegression(C=1e12, tol=1e-12, max_iter=10000).fit(x, y)
    assert abs(r.theta[0] - lr.coef_[0, 0]) <= 1e-6 and abs(r.theta[2] - lr.intercept_[0]) <= 1e-6


def test_temperature_is_platt_with_c_forced_to_zero():
    p, y, _ = F.fit_set()
    Jt, Jp = RC.basis("temperature"), RC.basis("platt")
    np.testing.assert_array_equal(Jt[:, 0], Jp[:, 0])
    np.testing.assert_array_equal(Jp[:, 1], [0, 0, 1])
    r = RC.fit_recalibration(p, y, "temperature")
    _, g, H = RC.unpack_sums(_eager(p, y, None, r.theta[None], 1, "joint").numpy()[0, 0])
    # stationary along the platt scale direction, not along c
    assert abs(Jp[:, 0] @ g) / F.FIT_N <= 1e-8 and abs(Jp[:, 1] @ g) / F.FIT_N > 1e-4


@pytest.mark.parametrize("objective", RC.OBJECTIVES)
def test_mirror_symmetry(objective):
    """Exchanging (a, b) and negating c mirrors p -> 1 - p, y -> 1 - y (p on a grid where 1 - p is exact)."""
    rng = np.random.default_rng(4)
    p = (rng.integers(1, 1024, (3, 200)) / 1024.0).astype(np.float32)
    y = rng.integers(0, 2, 200)
    th = np.array([[0.8, 0.3, 0.4]])
    a, ab = (v.numpy()[0, 0] for v in _eager(p, y, None, th, 1, objective, return_abs=True))
    b = _eager(1 - p, 1 - y, None, th[:, [1, 0, 2]] * [1, 1, -1], 1, objective).numpy()[0, 0]
    #          n  n1 loss g_a g_b g_c  aa ab ac  bb bc cc
    src = [0, 1, 2, 4, 3, 5, 9, 7, 10, 6, 8, 11]
    sign = np.array([1, 1, 1, 1, 1, -1, 1, 1, -1, 1, -1, 1.0])
    assert b[1] == a[0] - a[1]
    assert np.all(np.abs(b[2:] - (sign * a[src])[2:]) <= 2 * allowance(a, ab[src], 3)[2:])


def test_separable_set_returns_unconverged_with_a_warning():
    p = np.array([[0.2, 0.3, 0.7, 0.8]], np.float32)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        r = RC.fit_recalibration(p, np.array([0, 0, 1, 1]), "temperature")
    assert not r.converged and np.all(np.isfinite(r.theta)) and r.n_iter <= RC.MAX_ITER
    # margins so small that the scale passes 1e3 before the gradient vanishes
    p = np.array([[0.4999, 0.4998, 0.5001, 0.5002]], np.float32)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        r = RC.fit_recalibration(p, np.array([0, 0, 1, 1]), "platt")
    assert not r.converged and np.all(np.isfinite(r.theta)) and r.n_iter <= RC.MAX_ITER


def test_one_class_raises():
    p, _ = F.ensemble(50, 3)
    with pytest.raises(ValueError, match="both classes"):
        RC.fit_recalibration(p, np.ones(50, np.int64))
    y = np.zeros(50, np.int64)
    y[0] = 2
    with pytest.raises(ValueError, match="both classes"):
        RC.fit_recalibration(p, y)
    with pytest.raises(ValueError):
        RC.fit_recalibration(p, np.ones(50), method="isotonic")


def test_nonmonotone_beta_fit_is_constrained():
    rng = np.random.default_rng(0)
    lv = rng.integers(0, 3, 900)
    p = np.array([0.1, 0.5, 0.9], np.float32)[lv][None]
    y = (rng.random(900) < np.array([0.2, 0.8, 0.6])[lv]).astype(np.int64)
    free = RC.golden_fit(p, y, "beta")
    assert free["theta"][1] < 0          # the unconstrained optimum is not monotone
    r = RC.fit_recalibration(p, y, "beta")
    assert r.constrained == ("b",) and r.theta[1] == 0.0 and r.theta[0] > 0 and r.converged
    g = RC.golden_fit(p, y, "beta", fixed=("b",))
    bound = 2e-8 * g["n_valid"] / np.linalg.eigvalsh(g["H"])[0]
    assert np.max(np.abs(r.theta - g["theta"])) <= bound
    q = r.apply(np.array([[0.1, 0.5, 0.9]], np.float32))[0, :, 0]
    assert q[0] < q[1] < q[2]


@pytest.fixture(scope="module")
def crossfit():
    p, y, pid = F.fit_set()
    return RC.cross_recalibrate(p, y, pid, F.FIT_FOLDS, "beta", "joint", seed=2025)


def test_cross_recalibrate_folds(crossfit):
    p, y, pid = F.fit_set()
    cal, info = crossfit
    codes = F.fold_facts()
    np.testing.assert_array_equal(info["fold"], codes)
    assert cal.shape == (F.FIT_T, F.FIT_N, 1) and cal.dtype == np.float32
    for q in np.unique(pid):                       # folds never split a patient
        assert len(np.unique(codes[pid == q])) == 1
    assert sorted(np.unique(codes)) == list(range(F.FIT_FOLDS))
    for f in range(F.FIT_FOLDS):
        tr = codes != f
        g = RC.golden_fit(p[:, tr], y[tr], "beta")
        eig = np.linalg.eigvalsh(g["H"])
        assert eig[0] > 0 and g["theta"][0] >= 0 and g["theta"][1] >= 0
        one = RC.fit_recalibration(p[:, tr], y[tr], "beta")
        bound = F.theta_bound(g)
        assert np.max(np.abs(info["theta"][f] - one.theta)) <= bound
        assert np.max(np.abs(info["theta"][f] - g["theta"])) <= bound
        # every window of the fold is mapped by the fold's own theta: the emulation with that theta exactly, the
        # golden within one fp32 rounding
        own = recal.apply_eager(_t(p[:, ~tr]), None, _t(info["theta"][f][None])).numpy()
        np.testing.assert_array_equal(cal[:, ~tr, 0], own)
        gold = RC.golden_apply(p[:, ~tr], info["theta"][f]).astype(np.float64)
        assert np.max(np.abs(cal[:, ~tr, 0].astype(np.float64) - gold)) <= 2.0 ** -24
    assert all(info["converged"]) and info["nll_after"] < info["nll_before"]
    mean = cal[..., 0].astype(np.float64).mean(0)
    ref = C.golden_calibration(mean, y)["nll"]
    assert abs(info["nll_after"] - ref) < 1e-6     # the held-out loss is the NLL of the calibrated pooled mean


def test_assign_folds_and_a_complement_without_a_class():
    a = RC.assign_folds(None, 3, 1, n=10)
    assert a.dtype == np.int32 and sorted(np.bincount(a)) == [3, 3, 4]
    np.testing.assert_array_equal(a, RC.assign_folds(np.arange(10) * 5, 3, 1))
    ids = np.array(["b", "a", "b", "c", "a"])
    f = RC.assign_folds(ids, 2, 7)
    perm = np.random.default_rng(7).permutation(3)
    want = {np.array(["a", "b", "c"])[perm[r]]: r % 2 for r in range(3)}
    assert [want[i] for i in ids] == list(f)
    p, _ = F.ensemble(40, 2)
    y = np.zeros(40, np.int64)
    y[:3] = 1
    with pytest.raises(ValueError, match="both classes"):
        RC.cross_recalibrate(p, y, fold=np.r_[np.zeros(10), np.ones(30)].astype(np.int32), n_folds=2)


def test_evaluate_recalibration(tmp_path):
    p, y, pid = F.fit_set()
    B = 12
    res, det = RC.evaluate_recalibration(p, y, "fixture", patient_ids=pid, n_folds=F.FIT_FOLDS, method="platt",
                                         n_bootstrap=B, random_state=2025, output_plot_dir=str(tmp_path),
                                         return_details=True)
    for m in RC.METRICS:
        for sfx in ("before", "after", "diff", "diff_mean", "diff_ci_lower", "diff_ci_upper", "share_improved"):
            assert f"{m}_{sfx}" in res
        assert res[f"{m}_diff"] == res[f"{m}_after"] - res[f"{m}_before"]
        assert res[f"{m}_diff_ci_lower"] <= res[f"{m}_diff_mean"] <= res[f"{m}_diff_ci_upper"]
    assert res["ece_after"] < res["ece_before"] and res["nll_share_improved"] == 1.0
    assert {"theta_a_fold0", "theta_c_fold4", "fit_nll_before", "fit_nll_after", "converged"} <= set(res)
    assert C.plt is None or os.path.exists(tmp_path / "reliability_recalibrated_fixture.png")
    # the replicate-wise differences are after minus before on the same literal resamples
    idx = det["idx"].numpy()
    assert idx.shape == (B, F.FIT_N)
    mean = [C.per_window(x, "pred_variance")[0].numpy().astype(np.float64) for x in (p, det["calibrated"])]
    ref = [C.golden_replicates(m, m, y, np.zeros(0), idx) for m in mean]
    for m in RC.METRICS:
        tol = 2.0 / (calib.NLL_SCALE if m == "nll" else calib.P_SCALE)
        assert np.max(np.abs(det["replicates"][m] - (ref[1][m] - ref[0][m]))) <= tol, m
    # with a fit set the map is fitted there
    res2 = RC.evaluate_recalibration(p[:, :400], y[:400], "held", fit_predictions=p[:, 400:], fit_y=y[400:],
                                     method="temperature", n_bootstrap=0, make_plots=False)
    one = RC.fit_recalibration(p[:, 400:], y[400:], "temperature")
    assert res2["theta_a"] == one.theta[0] and res2["temperature"] == one.temperature
    assert "ece_diff_mean" not in res2 and res2["nll_after"] < res2["nll_before"]


def test_save_load_round_trip(tmp_path):
    p, y, _ = F.fit_set()
    r = RC.fit_recalibration(p, y, "beta", "member")
    path = r.save(str(tmp_path / "state"))
    assert path.endswith(".npz")
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"theta", "meta"}
    s = RC.Recalibrator.load(path)
    np.testing.assert_array_equal(s.theta, r.theta)
    assert s.scalars() == r.scalars()
    np.testing.assert_array_equal(s.apply(p), r.apply(p))


def test_apply_keeps_kind_and_shape():
    p, y, _ = F.fit_set()
    r = RC.fit_recalibration(p, y, "beta")
    a = r.apply(p[..., None])
    assert isinstance(a, np.ndarray) and a.shape == (F.FIT_T, F.FIT_N, 1) and a.dtype == np.float32
    b = r.apply(torch.from_numpy(p))
    assert isinstance(b, torch.Tensor) and b.device.type == "cpu" and b.dtype == torch.float32
    np.testing.assert_array_equal(a, b.numpy())
    d = np.abs(a[..., 0].astype(np.float64) - RC.golden_apply(p, r.theta).astype(np.float64))
    assert d.max() <= 2.0 ** -24
    q = p.copy()
    q[2, 5] = np.nan
    out = recal.apply_eager(_t(q), _t(np.r_[np.int32(7), np.zeros(F.FIT_N - 1, np.int32)]),
                            _t(np.tile(r.theta, (2, 1)))).numpy()
    assert np.isnan(out[2, 5]) and np.isnan(out[:, 0]).all() and np.isfinite(np.delete(out, [0, 5], axis=1)).all()
    ident = recal.apply_eager(_t(p), None, _t(RC.IDENTITY[None])).numpy()
    assert np.max(np.abs(ident.astype(np.float64) - np.clip(p.astype(np.float64), 1e-7, 1 - 1e-7))) <= 2.0 ** -24


def test_calibrated_set_feeds_the_other_analyses(crossfit, tmp_path):
    _, y, _ = F.fit_set()
    cal, _ = crossfit
    res = UT.evaluate_uq_methods(cal, y, "recal", n_bootstrap=3, random_state=1, output_plot_dir=str(tmp_path),
                                 make_plots=False)
    assert len(res) == 24 and all(np.isfinite(v) for v in res.values())
    cc = C.evaluate_calibration(cal, y, "recal", n_bootstrap=3, random_state=1, make_plots=False)
    assert np.isfinite(cc["ece"]) and np.isfinite(cc["nll"])
    assert UT.fit_recalibration is RC.fit_recalibration and UT.cross_recalibrate is RC.cross_recalibrate


def test_limits_raise():
    p, y = F.ensemble(10, 2)
    th = F.candidates(2)
    with pytest.raises(ValueError):
        _eager(np.zeros((129, 4), np.float32), y[:4], None, th, 1, "joint")
    with pytest.raises(ValueError):
        _eager(p, y, None, F.candidates(65), 1, "joint")
    with pytest.raises(ValueError):
        _eager(p, y, np.zeros(10, np.int32), th, 17, "joint")
    with pytest.raises(ValueError):
        _eager(p, y, None, th, 2, "joint")
    with pytest.raises(ValueError):
        _eager(p, y, None, th, 1, "pooled")
    with pytest.raises(ValueError):
        _eager(p.astype(np.float64), y, None, th, 1, "joint")
    assert recal.range_len(1) == 256 and recal.range_len(65536) == 256 and recal.range_len(65537) == 320
    assert recal.range_len(1 << 20) == 4096 and recal.q_chunk(50, 1, 1 << 20) == 64
    assert recal.lds_bytes(128, 16, recal.q_chunk(128, 16, 1000)) <= recal.LDS_LIMIT
    assert recal.lds_bytes(128, 16, recal.q_chunk(128, 16, 1000) + 1) > recal.LDS_LIMIT


def test_cli_end_to_end(tmp_path):
    import pandas as pd

    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli.commands import COMMANDS

    p, y, pid = F.fit_set()
    csv, raw = tmp_path / "detail.csv", tmp_path / "raw.npy"
    pd.DataFrame({"Patient_ID": pid, "True_Label": y, "Predicted_Probability": p.mean(0)}).to_csv(csv, index=False)
    np.save(raw, p[..., None])
    out_raw, out_csv, state = tmp_path / "cal.npy", tmp_path / "m.csv", tmp_path / "state.npz"
    table = COMMANDS["analyze_recalibration"]([
        "--input_csv", str(csv), "--raw_pred", str(raw), "--method", "platt", "--folds", "4", "--n_bootstrap", "5",
        "--seed", "3", "--output_raw_pred", str(out_raw), "--output_csv", str(out_csv),
        "--output_plot_dir", str(tmp_path), "--no_plots"])
    cal = np.load(out_raw)
    assert cal.shape == (F.FIT_T, F.FIT_N, 1) and cal.dtype == np.float32
    want, _ = RC.cross_recalibrate(p, y, pid, 4, "platt", seed=3)
    np.testing.assert_array_equal(cal, want)
    saved = pd.read_csv(out_csv)
    assert list(saved["metric"]) == list(table["metric"]) and "ece" in set(saved["metric"])
    row = saved.set_index("metric").loc["nll"]
    assert row["after"] < row["before"] and abs(row["diff"] - (row["after"] - row["before"])) < 1e-12
    # with a fit set: one map, saved as a state that loads back
    COMMANDS["analyze_recalibration"]([
        "--input_csv", str(csv), "--raw_pred", str(raw), "--fit_csv", str(csv), "--fit_raw_pred", str(raw),
        "--method", "beta", "--n_bootstrap", "0", "--output_raw_pred", str(out_raw), "--output_csv", str(out_csv),
        "--state", str(state), "--no_plots"])
    st = RC.Recalibrator.load(str(state))
    np.testing.assert_array_equal(np.load(out_raw), st.apply(p))
    assert np.max(np.abs(st.theta - F.golden_facts("beta", "joint")["theta"])) <= F.theta_bound(
        F.golden_facts("beta", "joint"))


def _fit_rank(rank, world):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.parallel import comm

    p, y, _ = F.fit_set()
    meter = comm.CommMeter()
    with comm.metering(meter):
        r = RC.fit_recalibration(p, y, "beta")
    return r.theta, r.nll_after, r.n_iter, r.n_valid, meter.summary()


def test_two_rank_fit_matches_one_rank():
    p, y, _ = F.fit_set()
    one = RC.fit_recalibration(p, y, "beta")
    bound = F.theta_bound(F.golden_facts("beta", "joint"))
    for theta, nll, n_iter, nv, summary in run_ranks(_fit_rank, 2):
        assert nv == one.n_valid == F.FIT_N
        assert np.max(np.abs(theta - one.theta)) <= bound and abs(nll - one.nll_after) <= 1e-12
        ops = {op: v for ph in summary["phases"].values() for op, v in ph.items()}
        # one all-reduce per evaluation: the start and one per iteration
        assert list(ops) == ["recal_all_reduce"] and ops["recal_all_reduce"]["count"] == n_iter + 1
