"""Last-layer Laplace on the GPU: ``csrc/uq_laplace.hip`` against the torch float64 emulations on the same fp32
features, grid invariance of the Gram kernel, the engine's feature path and the fit / predict round trip.

Allowances come from the float64 reference's own term sums (``laplace_fixtures``), never from the kernel."""
import dataclasses

import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.cnn import AlarconCNN1D
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import laplace as L
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import laplace as UL

from . import laplace_fixtures as F

pytestmark = pytest.mark.gpu

GRAM_D = [3, 16, 96, 100, 127]
GRAM_N = [1, 15, 16, 17, 255, 256, 257, 1000, 20001]


def _dev():
    _ext.require()
    return torch.device("cuda")


def _check_gram(phi, theta, y, grid=0):
    dev = _dev()
    pt, tt, yt = torch.from_numpy(phi).to(dev), torch.from_numpy(theta).to(dev), torch.from_numpy(y).to(dev)
    got = L.gram(pt, tt, yt, grid=grid)
    ref = L.gram_eager(pt, tt, yt)
    al = F.gram_allowance(phi, theta, y)
    H, Hr = got["H"].cpu().numpy(), ref["H"].cpu().numpy()
    g, gr = got["g"].cpu().numpy(), ref["g"].cpu().numpy()
    eh = np.abs(H - Hr) - al["H"]
    eg = np.abs(g - gr) - al["g"]
    print(f"max |dH| {np.abs(H - Hr).max():.3e} (allowance at it {al['H'].flat[np.argmax(eh)]:.3e}), "
          f"max |dg| {np.abs(g - gr).max():.3e}, dloglik {abs(got['loglik'] - ref['loglik']):.3e} "
          f"(allowance {al['loglik']:.3e})")
    assert got["n_valid"] == ref["n_valid"] == al["n_valid"] and got["n_total"] == len(y)
    assert np.array_equal(H, H.T), "H is not exactly symmetric"
    assert np.isfinite(H).all() and np.isfinite(g).all()
    assert eh.max() <= 0.0, f"H exceeds its allowance by {eh.max():.3e}"
    assert eg.max() <= 0.0, f"g exceeds its allowance by {eg.max():.3e}"
    assert abs(got["loglik"] - ref["loglik"]) <= al["loglik"]
    return got


@pytest.mark.parametrize("n", GRAM_N)
@pytest.mark.parametrize("D", GRAM_D)
def test_gram_matches_eager(D, n):
    phi, y, _ = F.spoil(F.make_features(n, D), F.make_labels(n))
    _check_gram(phi, F.make_theta(D), y)


@pytest.mark.parametrize("kind", F.KINDS)
def test_gram_fixture_kinds(kind):
    D = 96
    n = 60 if kind == "onehot" else 1000
    got = _check_gram(F.make_features(n, D, kind), F.make_theta(D, kind), F.make_labels(n))
    assert got["n_valid"] == n
    if kind == "saturated":
        assert float(got["H"].abs().max()) < 1e-10  # every weight is ~4e-18 or 0


def test_gram_grid_invariance():
    dev = _dev()
    D, n = 96, 20001
    assert L.n_ranges(n, D) >= 3
    phi, y, _ = F.spoil(F.make_features(n, D), F.make_labels(n))
    pt, tt, yt = torch.from_numpy(phi).to(dev), torch.from_numpy(F.make_theta(D)).to(dev), torch.from_numpy(y).to(dev)
    base = L.gram_flat(pt, tt, yt)
    for grid in (1, 3, 0):
        again = L.gram_flat(pt, tt, yt, grid=grid)
        assert torch.equal(base, again), f"grid {grid}: not bitwise equal"
    # several ranges at a small n through the range hook: still grid invariant, and within the allowance
    small = L.gram_flat(pt[:300], tt, yt[:300], rlen=64)
    assert L.n_ranges(300, D, 64) == 5 and L.bytes_partial(300, D, 64) == 5 * L.partial_doubles(D) * 8
    assert torch.equal(small, L.gram_flat(pt[:300], tt, yt[:300], grid=2, rlen=64))
    ref = L.gram_flat_eager(pt[:300], tt, yt[:300])
    al = F.gram_allowance(phi[:300], F.make_theta(D), y[:300])
    d = (small - ref).abs().cpu().numpy()
    assert (d[: (D + 1) ** 2].reshape(D + 1, D + 1) <= al["H"]).all()


def test_wide_head_takes_the_torch_path_with_one_warning():
    import warnings

    dev = _dev()
    D, n = 128, 50  # D + 1 = 129 > 128: no kernel instance
    assert not L.supports(D)
    phi, th, y = F.make_features(n, D), F.make_theta(D), F.make_labels(n)
    pt, tt, yt = torch.from_numpy(phi).to(dev), torch.from_numpy(th).to(dev), torch.from_numpy(y).to(dev)
    L._warned.discard(D)
    with pytest.warns(RuntimeWarning, match="no HIP kernel"):
        got = L.gram_flat(pt, tt, yt)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = L.gram_flat(pt, tt, yt)
    for other in (again, L.gram_flat_eager(pt, tt, yt)):  # the same torch code (its GEMM may reorder sums)
        assert torch.allclose(got, other, rtol=1e-12, atol=1e-300)


def _state(D, n_fit=400, lam=1.0):
    phi, th, y = F.make_features(n_fit, D), F.make_theta(D), F.make_labels(n_fit)
    g = UL.golden_laplace_fit(phi, th, y)
    return UL.state_from_sums(th, g["H"], g["g"], g["loglik"], g["n_valid"], g["n_total"], lam)


@pytest.mark.parametrize("T", [0, 1, 7, 50, 200])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("D", [3, 96, 127])
def test_predict_matches_eager(D, n, T):
    dev = _dev()
    if D == 96 and T == 200:
        assert L.col_blocks(D, T) > 1  # more than one LDS block of [theta | M]
    st = _state(D)
    phi = F.make_features(n, D, seed=17)
    if n >= 63:
        phi[1, 0] = np.nan
        phi[n - 2, D - 1] = -np.inf
    z = UL.draws(T, D + 1, 3)
    pt = torch.from_numpy(phi).to(dev)
    got = UL.predict_features(pt, st, z)
    ref = UL.predict_features(pt, st, z, eager=True)
    al = F.predict_allowance(phi, st.theta, st.chol)
    bad = al["bad"]
    assert got[0].shape == (T, n) and got[0].dtype == torch.float32
    for name, a, b in zip(("preds", "mu", "v", "probit"), got, ref):
        a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(a), np.broadcast_to(bad, a.shape)), f"{name}: NaN pattern"
        d = np.abs(a - b)[..., ~bad]
        lim = al[name] if np.isscalar(al[name]) else al[name][~bad]
        if d.size:
            print(f"{name}: max |d| {d.max():.3e}")
            assert (d <= lim).all(), f"{name}: exceeds its allowance by {(d - lim).max():.3e}"


def _model(seed=5, spec=SPEC, dev="cuda"):
    return AlarconCNN1D(spec=spec, params=R.synthetic_params(spec, seed), device=dev)


def _x(n, seed):
    return torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("n", [48, 130])
def test_engine_features(n):
    _dev()
    model = _model()
    assert model.uses_x3()
    x = _x(n, n)
    phi = model.last_layer_features(x)
    D = SPEC.final_channels
    assert phi.shape == (n, D) and phi.dtype == torch.float32 and phi.is_cuda
    th = UL.head_theta(model)
    f = phi.double().cpu().numpy() @ th[:D] + th[D]
    p_feat = 1.0 / (1.0 + np.exp(-f))
    p_model = model.predict(x).reshape(-1).astype(np.float64)
    bound = 0.25 * (D + 4) * 2.0 ** -24 * (np.abs(phi.double().cpu().numpy() * th[:D]).sum(axis=1)) + 2.0 ** -23
    d = np.abs(p_feat - p_model)
    print(f"features vs predict: max |dp| {d.max():.3e} (bound at it {bound[np.argmax(d - bound)]:.3e})")
    assert (d <= bound).all()
    pc = {k: v.detach().cpu().float() for k, v in model.params.items()}
    r32 = R.forward(SPEC, pc, x).reshape(-1).double().numpy()
    print(f"features vs fp32 reference: max |dp| {np.abs(p_feat - r32).max():.3e}")
    assert np.abs(p_feat - r32).max() <= 1e-5
    chunked = model.last_layer_features(x, max_samples=-(-n // 3))
    rel = ((chunked - phi).abs() / phi.abs().clamp(min=1e-30)).max().item()
    scale = (chunked - phi).abs().max().item() / phi.abs().max().item()
    print(f"chunked vs unchunked: max relative {rel:.3e}, relative to the largest feature {scale:.3e}")
    assert ((chunked - phi).abs() <= 1e-6 * phi.abs()).all()


def test_fallback_features_pooled():
    _dev()
    pooled = dataclasses.replace(SPEC, blocks=tuple(dataclasses.replace(b, pool=(i < 5))
                                                   for i, b in enumerate(SPEC.blocks)))
    model = _model(9, pooled)
    assert not model.uses_x3()
    x = _x(40, 2)
    phi = model.last_layer_features(x)
    th = UL.head_theta(model)
    D = pooled.final_channels
    p = 1.0 / (1.0 + np.exp(-(phi.double().cpu().numpy() @ th[:D] + th[D])))
    d = np.abs(p - model.predict(x).reshape(-1).astype(np.float64)).max()
    print(f"fallback features vs predict: max |dp| {d:.3e}")
    assert d <= 1e-6


@pytest.fixture(scope="module")
def e2e():
    """512 fit / 130 test windows: the device fit and prediction, and the golden ones on the float64 and on the
    fp32 PyTorch reference model's features."""
    _ext.require()
    model = _model(21)
    xf, xt = _x(512, 31), _x(130, 32)
    yf = F.make_labels(512)
    out = {"model": model, "xf": xf, "xt": xt, "yf": yf}
    p32 = {k: v.detach().cpu().float() for k, v in model.params.items()}
    p64 = {k: v.double() for k, v in p32.items()}
    feats = {}
    with torch.no_grad():
        for tag, p, dt in (("f64", p64, torch.float64), ("f32", p32, None)):
            feats[tag] = [R.forward(SPEC, p, x, dtype=dt, return_features=True).numpy() for x in (xf, xt)]
    th = UL.head_theta(model)
    for tag in ("f64", "f32"):
        g = UL.golden_laplace_fit(feats[tag][0], th, yf)
        st = UL.state_from_sums(th, g["H"], g["g"], g["loglik"], g["n_valid"], g["n_total"], 1.0)
        out[tag] = {"fit": g, "state": st, "pred": UL.golden_laplace_predict(feats[tag][1], st, 50, 2025)}
    out["feats"] = feats
    st = UL.fit_laplace(model, xf.numpy(), yf, prior_precision=1.0)
    out["dev"] = {"state": st, "pred": UL.laplace_predict(model, st, xt.numpy(), 50, 2025, return_moments=True)}
    return out


def test_end_to_end_against_golden(e2e):
    """The allowance is not derivable (engine deviation propagated through a matrix inverse): the deviation of the
    fp32 PyTorch feature path from the float64 one is measured here, and 4x that plus the kernel-level
    allowance is allowed."""
    g64, g32, dev = e2e["f64"], e2e["f32"], e2e["dev"]
    st = dev["state"]
    assert st.n_valid == 512 and st.n_total == 512 and st.prior_precision == 1.0
    th = st.theta
    ka = F.gram_allowance(e2e["feats"]["f64"][0].astype(np.float32), th, e2e["yf"])
    pa = F.predict_allowance(e2e["feats"]["f64"][1].astype(np.float32), th, g64["state"].chol)
    preds, mom = dev["pred"]
    assert preds.shape == (50, 130, 1) and preds.dtype == np.float32
    rows = [("H", st.H, g64["fit"]["H"], g32["fit"]["H"], ka["H"].max()),
            ("v", mom["logit_variance"], g64["pred"][1]["logit_variance"], g32["pred"][1]["logit_variance"],
             pa["v"].max()),
            ("preds", preds[..., 0].astype(np.float64), g64["pred"][0].astype(np.float64),
             g32["pred"][0].astype(np.float64), pa["preds"])]
    for name, got, ref, ref32, kernel in rows:
        measured = np.abs(ref32 - ref).max()
        d = np.abs(got - ref).max()
        print(f"{name}: device vs golden(f64 features) {d:.3e}; fp32 PyTorch features vs f64 {measured:.3e}; "
              f"kernel allowance {kernel:.3e}")
        assert d <= 4.0 * measured + kernel, name


def test_auto_prior_agrees_with_golden(e2e):
    auto_dev = e2e["dev"]["state"].with_prior_precision("auto")
    auto_gold = e2e["f64"]["state"].with_prior_precision("auto")
    d = abs(np.log(auto_dev.prior_precision) - np.log(auto_gold.prior_precision))
    print(f"auto lambda: device {auto_dev.prior_precision:.6g}, golden {auto_gold.prior_precision:.6g}")
    assert d <= 1e-3
    assert auto_dev.prior_precision_at_bound == auto_gold.prior_precision_at_bound


def test_consumers_take_the_prediction_set_on_device(e2e):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration, discrimination
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import uq_techniques as U

    model, st = e2e["model"], e2e["dev"]["state"]
    preds = U.laplace_predict(model, st, e2e["xt"].numpy(), n_samples=20, as_numpy=False)
    assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.shape == (20, 130, 1)
    y = F.make_labels(130)

    def finite(d):
        for k, v in d.items():
            assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k

    finite(U.uq_evaluation_dist(preds, y))
    boots = U.bootstrap_metrics(preds, y, n_bootstrap=8, parity=False)
    assert len(boots) == 8
    for b in boots:
        finite(b)
    cal = calibration.calibration_metrics(preds, y)
    finite({k: cal[k] for k in ("ece", "mce", "brier", "nll")})  # the per-bin arrays are NaN for empty bins
    assert int(np.sum(cal["bin_count"])) == 130
    finite(discrimination.discrimination_metrics(preds, y))
