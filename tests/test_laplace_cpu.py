"""Last-layer Laplace without a GPU: the torch float64 emulation against the NumPy golden, evidence, posterior,
sampling, the state file, the model-level API, the CLI and the 2-rank fit."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.cnn import AlarconCNN1D
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import laplace as L
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import laplace as UL

from . import laplace_fixtures as F
from .dist_utils import run_ranks


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _state(D=16, n=300, lam=1.0, kind="gauss"):
    phi, th, y = F.make_features(n, D, kind), F.make_theta(D, kind), F.make_labels(n)
    g = UL.golden_laplace_fit(phi, th, y)
    return UL.state_from_sums(th, g["H"], g["g"], g["loglik"], g["n_valid"], g["n_total"], lam), phi, y


@pytest.mark.parametrize("n", [1, 50, 1000])
@pytest.mark.parametrize("D", [3, 16, 96, 100])
@pytest.mark.parametrize("kind", F.KINDS)
def test_gram_eager_matches_golden(kind, D, n):
    phi, y, spoiled = F.spoil(F.make_features(n, D, kind), F.make_labels(n))
    th = F.make_theta(D, kind)
    got = L.gram_eager(_t(phi), _t(th), _t(y))
    ref = UL.golden_laplace_fit(phi, th, y)
    assert got["n_valid"] == ref["n_valid"] == n - spoiled and got["n_total"] == ref["n_total"] == n
    al = _vs_golden_allowance(phi, th, y)
    H = got["H"].numpy()
    assert np.array_equal(H, H.T)
    assert (np.abs(H - ref["H"]) <= al["H"]).all()
    assert (np.abs(got["g"].numpy() - ref["g"]) <= al["g"]).all()
    assert abs(got["loglik"] - ref["loglik"]) <= al["loglik"]


def _vs_golden_allowance(phi, th, y):
    """Emulation against golden: two float64 formulations of the same sums, so twice the order allowance; and the
    golden forms the logit as a BLAS dot product, the emulation in the kernel's order, so the two logits of a
    window differ by up to ``df = (D + 2) 2^-52 sum_c |theta_c phi~_c|``.  A weight or a residual moves by at most
    ``df`` relative to itself (``|d log w / df| = |1 - 2p| <= 1``, ``|dr / df| = w <= |r|``), a log-likelihood term by
    at most ``df`` absolutely (``|d ll / df| <= 1``)."""
    al, tb = F.gram_allowance(phi, th, y), F.term_bound(phi, th, y)
    x = np.where(np.isfinite(phi), phi, 0.0).astype(np.float64)
    df = (phi.shape[1] + 2) * 2.0 ** -52 * ((np.abs(x) @ np.abs(th[:-1]) + abs(th[-1])).max() if len(x) else 0.0)
    return {"H": 2 * al["H"] + df * tb["H"], "g": 2 * al["g"] + df * tb["g"],
            "loglik": 2 * al["loglik"] + df * tb["n_valid"]}


def test_logits_eager_order_is_the_documented_one():
    D, n = 10, 7
    phi, th = F.make_features(n, D), F.make_theta(D)
    x = phi.astype(np.float64)
    a = [np.zeros(n) for _ in range(4)]
    for c in range(D):
        a[c % 4] = a[c % 4] + th[c] * x[:, c]
    f = ((a[0] + a[1]) + (a[2] + a[3])) + th[D]
    assert np.array_equal(L.logits_eager(_t(x), _t(th)).numpy(), f)


@pytest.mark.parametrize("kind", ["gauss", "tiny", "large", "onehot"])
def test_loglik_equals_sklearn_log_loss(kind):
    from scipy.special import expit
    from sklearn.metrics import log_loss

    D, n = 16, 50
    phi, th, y = F.make_features(n, D, kind), F.make_theta(D, kind), F.make_labels(n)
    p = expit(np.concatenate([phi.astype(np.float64), np.ones((n, 1))], axis=1) @ th)
    want = -log_loss(y, p, normalize=False, labels=[0, 1])
    for got in (UL.golden_laplace_fit(phi, th, y)["loglik"], L.gram_eager(_t(phi), _t(th), _t(y))["loglik"]):
        assert abs(got - want) <= 1e-10 * abs(want)


def test_range_rule():
    assert L.range_len(20001, 96) == L.MIN_RANGE and L.n_ranges(20001, 96) >= 3
    for D in (3, 96, 127):
        for n in (1, 10 ** 6, 10 ** 8):
            assert L.bytes_partial(n, D) <= L.PARTIAL_LIMIT
            assert L.range_len(n, D) % L.TILE_WINDOWS == 0
    assert L.col_blocks(96, 200) > 1 and L.col_blocks(3, 0) == 1
    assert L.supports(127) and not L.supports(128)


# ------------------------------------------------------------------------------------------------ evidence
def _evidence_case(scale=1.0, theta_scale=1.0, D=16, n=300):
    phi, th, y = F.make_features(n, D) * np.float32(scale), F.make_theta(D) * theta_scale, F.make_labels(n)
    g = UL.golden_laplace_fit(phi, th, y)
    return np.clip(np.linalg.eigvalsh(g["H"]), 0, None), th, g["loglik"]


def test_prior_optimum_beats_brute_force_and_is_stationary():
    eig, th, ll = _evidence_case()
    lam, logz, at_bound = UL.optimize_prior_precision(eig, th, ll)
    assert not at_bound and UL.PRIOR_MIN < lam < UL.PRIOR_MAX
    grid = np.exp(np.linspace(np.log(UL.PRIOR_MIN), np.log(UL.PRIOR_MAX), 400))
    assert logz >= max(UL.log_evidence(l, eig, th, ll) for l in grid)
    h = 1e-4
    d = (UL.log_evidence(lam * np.exp(h), eig, th, ll) - UL.log_evidence(lam * np.exp(-h), eig, th, ll)) / (2 * h)
    assert abs(d) <= 1e-6 * abs(logz)
    assert logz == UL.log_evidence(lam, eig, th, ll)


def test_prior_runs_to_each_bound():
    eig, th, ll = _evidence_case()
    # a huge head: -lambda |theta|^2 / 2 dominates, the evidence falls with lambda everywhere
    lam, _, at = UL.optimize_prior_precision(eig, th * 1e5, ll)
    assert at and lam == UL.PRIOR_MIN
    # a zero head and no curvature: (D + 1) / 2 log lambda - 1/2 sum log(lambda) is flat, a tiny head tips it up
    lam, _, at = UL.optimize_prior_precision(np.zeros_like(eig) + 1e9, th * 1e-9, ll)
    assert at and lam == UL.PRIOR_MAX
    for l in np.exp(np.linspace(np.log(UL.PRIOR_MIN), np.log(UL.PRIOR_MAX), 400)):
        assert UL.log_evidence(UL.PRIOR_MAX, np.zeros_like(eig) + 1e9, th * 1e-9, ll) >= \
            UL.log_evidence(l, np.zeros_like(eig) + 1e9, th * 1e-9, ll)


# ------------------------------------------------------------------------------------------------ posterior
def test_posterior_factor_and_large_prior_limit():
    st, phi, _ = _state(D=16, lam=1.0)
    d1 = st.theta.size
    P = st.H + st.prior_precision * np.eye(d1)
    assert np.abs(st.chol @ st.chol.T @ P - np.eye(d1)).max() <= 1e-9
    big = st.with_prior_precision(1e12)
    preds, mom = UL.golden_laplace_predict(phi, big, 20, 4)
    xt = np.concatenate([phi.astype(np.float64), np.ones((len(phi), 1))], axis=1)
    want = (xt * xt).sum(axis=1) / 1e12
    assert (np.abs(mom["logit_variance"] - want) <= 1e-6 * want).all()
    assert np.abs(preds - mom["map_prob"][None, :]).max() <= 1e-5
    p2 = UL.predict_features(_t(phi), big, UL.draws(20, d1, 4))
    assert (np.abs(p2[2].numpy() - want) <= 1e-6 * want).all()
    assert np.abs(p2[0].numpy() - mom["map_prob"][None, :]).max() <= 1e-5


@pytest.mark.parametrize("D", [3, 16, 96])
def test_identity_draws_tie_samples_to_variance(D):
    """z = I: sample t is theta + L[:, t], so sum_t (logit_t - mu)^2 = |L^T phi~|^2 = v -- the sample columns and the
    variance columns are built from the same L."""
    st, _, _ = _state(D=D)
    phi = F.make_features(40, D, seed=23)
    lg, mu, v, _ = UL.predict_features(_t(phi), st, np.eye(D + 1), return_logits=True)
    lg, mu, v = lg.numpy(), mu.numpy(), v.numpy()
    al = F.predict_allowance(phi, st.theta, st.chol)
    tb = F.predict_term_bound(phi, st.theta, st.chol)
    # logit_t - mu cancels mu: every difference carries the rounding of both logits, (D + 17) 2^-52 |theta . phi~| terms
    psi = lg - mu[None, :]
    extra = 2.0 * np.abs(psi).sum(axis=0) * 2.0 * al["mu"] + (D + 17) * 2.0 ** -52 * tb["v"]
    assert (np.abs((psi ** 2).sum(axis=0) - v) <= al["v"] + extra).all()
    gp, gm = UL.golden_laplace_predict(phi, st, 5, 1)
    assert (np.abs(gm["logit_variance"] - v) <= 2 * al["v"]).all() and (np.abs(gm["mean_logit"] - mu) <= 2 * al["mu"]).all()


def test_sampling_is_a_pure_prefix_stable_function():
    d1 = 17
    assert np.array_equal(UL.draws(50, d1, 2025)[:7], UL.draws(7, d1, 2025))
    assert np.array_equal(np.random.default_rng(9).standard_normal((50, d1))[:7],
                          np.random.default_rng(9).standard_normal((7, d1)))
    st, phi, _ = _state(D=16)
    a = UL.predict_features(_t(phi), st, UL.draws(50, d1, 2025))[0]
    b = UL.predict_features(_t(phi), st, UL.draws(7, d1, 2025))[0]
    assert torch.equal(a[:7], b)
    ga, gb = UL.golden_laplace_predict(phi, st, 50, 2025)[0], UL.golden_laplace_predict(phi, st, 7, 2025)[0]
    assert np.array_equal(ga[:7], gb)
    assert np.abs(a.numpy() - ga).max() <= 2.0 ** -23
    assert not np.array_equal(ga[:7], UL.golden_laplace_predict(phi, st, 7, 2026)[0])


def test_predict_eager_nan_windows_and_moments_only():
    st, phi, _ = _state(D=16)
    phi = phi[:30].copy()
    phi[4, 3] = np.nan
    phi[9, 0] = np.inf
    for T in (0, 3):
        p, mu, v, pb = UL.predict_features(_t(phi), st, UL.draws(T, 17, 1))
        gp, gm = UL.golden_laplace_predict(phi, st, T, 1)
        assert p.shape == (T, 30) and gp.shape == (T, 30)
        bad = np.zeros(30, bool)
        bad[[4, 9]] = True
        for t in (mu, v, pb):
            assert np.array_equal(np.isnan(t.numpy()), bad)
        assert np.array_equal(np.isnan(p.numpy()), np.broadcast_to(bad, (T, 30)))
        assert np.array_equal(np.isnan(gp), np.broadcast_to(bad, (T, 30)))
        assert np.nanmax(np.abs(pb.numpy() - gm["probit_prob"])) <= 1e-12


# ------------------------------------------------------------------------------------------------ state
def test_state_roundtrip_and_refactorisation(tmp_path):
    st, phi, y = _state(D=16, lam="auto")
    st = dataclasses.replace(st, spec_json=SPEC.to_json(), weights_hash="ab" * 32)
    path = st.save(str(tmp_path / "state"))
    assert path.endswith(".npz")
    back = UL.LaplaceState.load(path)
    for f in dataclasses.fields(st):
        a, b = getattr(st, f.name), getattr(back, f.name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f.name
        else:
            assert type(a) is type(b) and a == b, f.name
    with np.load(path, allow_pickle=False) as z:  # nothing in the file needs pickle
        assert set(z.files) == {"theta", "H", "g", "chol", "scalars", "meta"}
    fresh, _, _ = _state(D=16, lam=3.5)
    moved = st.with_prior_precision(3.5)
    assert moved.prior_precision == 3.5 and not moved.prior_precision_at_bound
    for k in ("chol", "H", "g", "theta"):
        assert np.array_equal(getattr(moved, k), getattr(fresh, k)), k
    assert moved.log_evidence == fresh.log_evidence and moved.map_gradient_norm == fresh.map_gradient_norm
    assert moved.map_gradient_norm == float(np.linalg.norm(st.g + 3.5 * st.theta))
    with pytest.raises(ValueError):
        st.with_prior_precision(-1.0)


# ------------------------------------------------------------------------------------------------ model level
def _model(seed=5):
    return AlarconCNN1D(spec=SPEC, params=R.synthetic_params(SPEC, seed), device="cpu")


def _x(n, seed):
    return torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(seed)).numpy()


@pytest.fixture(scope="module")
def fitted():
    model = _model()
    x, y = _x(40, 1), F.make_labels(40)
    return model, x, y, UL.fit_laplace(model, x, y, prior_precision="auto")


def test_model_level_cpu(fitted, tmp_path, monkeypatch):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import drivers
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import uq_techniques as U

    monkeypatch.chdir(tmp_path)
    model, x, y, st = fitted
    assert st.n_valid == st.n_total == 40 and st.D == SPEC.final_channels
    assert st.weights_hash == UL.weights_hash(model) and st.spec_json == SPEC.to_json()
    phi = model.last_layer_features(x)
    assert phi.shape == (40, SPEC.final_channels) and phi.dtype == torch.float32
    gold = UL.golden_laplace_fit(phi.numpy(), st.theta, y)
    al = F.gram_allowance(phi.numpy(), st.theta, y)
    assert (np.abs(st.H - gold["H"]) <= _vs_golden_allowance(phi.numpy(), st.theta, y)["H"]).all()
    # chunked fit: float64 summation order only
    st3 = UL.fit_laplace(model, x, y, prior_precision=st.prior_precision, chunk_windows=17)
    assert st3.n_valid == 40 and (np.abs(st3.H - st.H) <= 2 * al["H"]).all()
    preds, mom = U.laplace_predict(model, st, x, n_samples=12, return_moments=True)
    assert preds.shape == (12, 40, 1) and preds.dtype == np.float32
    assert set(mom) == {"mean_logit", "logit_variance", "probit_prob", "map_prob"}
    assert np.abs(mom["map_prob"] - model.predict(x).reshape(-1)).max() <= 1e-6
    assert (mom["logit_variance"] > 0).all()
    res = U.evaluate_uq_methods(preds, y, "llla", n_bootstrap=5, random_state=1, make_plots=False)
    assert len(res) == 24
    out = drivers.evaluate_laplace(model, st, x, y, patient_ids=np.arange(40) // 10, model_eval_label="T",
                                   save_detailed_csv=True, n_samples=12, n_bootstrap=5, output_csv_dir="csv",
                                   output_plot_dir="plots", make_plots=False)
    import pandas as pd

    df = pd.read_csv("csv/detailed_results_T.csv")
    assert list(df.columns) == drivers.DETAIL_COLUMNS and len(df) == 40
    assert os.path.exists("laplace_raw_pred_T.npy") and np.load("laplace_raw_pred_T.npy").shape == (12, 40, 1)
    assert 0.0 <= out["probit_accuracy"] <= 1.0 and out["prior_precision"] == st.prior_precision
    assert out["n_valid"] == 40 and set(res) <= set(out)


def test_other_weights_are_refused(fitted):
    model, x, _, st = fitted
    other = _model(6)
    with pytest.raises(ValueError, match="weight"):
        UL.laplace_predict(other, st, x[:4], n_samples=2)
    UL.laplace_predict(model, st, x[:4], n_samples=2)


def test_return_features_is_the_pooled_activation():
    p = R.synthetic_params(SPEC, 3)
    x = torch.from_numpy(_x(6, 2))
    g = R.forward(SPEC, p, x, return_features=True)
    lg = R.forward(SPEC, p, x, return_logits=True)
    assert g.shape == (6, SPEC.final_channels)
    assert torch.equal(g @ p["output_layer/kernel"] + p["output_layer/bias"], lg)


def test_cli(tmp_path, monkeypatch):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import commands

    assert "analyze_laplace_patient_level" in commands.COMMANDS
    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import analyze_laplace_patient_level as mod

    assert mod.analyze_laplace_patient_level is commands.analyze_laplace_patient_level
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "data"
    d.mkdir()
    np.save(d / "X_train_win_std_smote.npy", _x(48, 3))
    np.save(d / "y_train_smote.npy", F.make_labels(48))
    np.save(d / "X_test_win_std_unbalanced.npy", _x(30, 4))
    np.save(d / "y_test_unbalanced.npy", F.make_labels(30))
    np.save(d / "patient_ids_test_unbalanced.npy", np.arange(30) // 10)
    np.save(d / "X_test_win_std_rus.npy", _x(20, 5))
    np.save(d / "y_test_rus.npy", F.make_labels(20))
    model = _model(8)
    mp = model.save(str(tmp_path / "m.keras"))
    argv = ["--data_dir", str(d), "--model_path", mp, "--n_samples", "6", "--n_bootstrap", "4", "--no_plots",
            "--state", str(tmp_path / "post" / "state.npz"), "--output_csv_dir", "csv", "--prior_precision", "2.5"]
    res = commands.analyze_laplace_patient_level(argv)
    st = UL.LaplaceState.load(str(tmp_path / "post" / "state.npz"))
    assert st.prior_precision == 2.5 and st.n_total == 48
    assert os.path.exists("csv/detailed_results_CNN_LLLA_Unbalanced.csv")
    for k in ("unbalanced", "balanced"):
        assert res[k]["prior_precision"] == 2.5 and "probit_accuracy" in res[k] and len(res[k]) > 24
    # a second run loads the state instead of fitting
    os.remove(d / "X_train_win_std_smote.npy")
    again = commands.analyze_laplace_patient_level(argv)
    assert again["balanced"]["log_evidence"] == res["balanced"]["log_evidence"]


# ------------------------------------------------------------------------------------------------ 2 ranks
def _fit_rank(rank, world):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.parallel import comm

    model = _model()
    x, y = _x(41, 7), F.make_labels(41)
    y[5] = 2
    meter = comm.CommMeter()
    with comm.metering(meter):
        st = UL.fit_laplace(model, x, y, prior_precision=1.0)
    return st, meter.summary()


def test_two_rank_fit_equals_one_rank():
    res = run_ranks(_fit_rank, 2)
    model = _model()
    x, y = _x(41, 7), F.make_labels(41)
    y[5] = 2
    one = UL.fit_laplace(model, x, y, prior_precision=1.0)
    al = F.gram_allowance(model.last_layer_features(x).numpy(), one.theta, y)
    assert one.n_valid == 40 and one.n_total == 41
    for st, summary in res:
        assert st.n_valid == one.n_valid and st.n_total == one.n_total
        assert (np.abs(st.H - one.H) <= al["H"]).all() and (np.abs(st.g - one.g) <= al["g"]).all()
        assert abs(st.loglik - one.loglik) <= al["loglik"]
        ops = {op: v for ph in summary["phases"].values() for op, v in ph.items()}
        assert list(ops) == ["laplace_all_reduce"] and ops["laplace_all_reduce"]["count"] == 1
