"""Seeded features, heads and labels for the last-layer Laplace tests, and the float64 term sums that the
kernel allowances are computed from (never from the output under test)."""
import numpy as np
from scipy.special import expit

KINDS = ("gauss", "saturated", "tiny", "large", "onehot")


def make_theta(D, kind="gauss", seed=11):
    """(D + 1,) float64 head: unit-scale logits on unit features ("large": on features of 1e4)."""
    rng = np.random.default_rng(seed + 7 * D)
    th = rng.standard_normal(D + 1) / np.sqrt(D + 1.0)
    if kind == "large":
        th[:D] *= 1e-4
    return th


def make_features(n, D, kind="gauss", seed=5):
    """(n, D) float32.  "saturated": the logits under make_theta(D, kind) are +-40 (p (1 - p) ~ 4e-18) and, for
    every fourth window, +-800 (exp underflows: p (1 - p) = 0); "tiny": ~1e-6; "large": ~1e4; "onehot": unit
    vectors, so H is rank deficient (and n < D + 1 where the test picks n so)."""
    rng = np.random.default_rng(seed + 1000 * D + n)
    if kind == "onehot":
        x = np.zeros((n, D))
        x[np.arange(n), np.arange(n) % D] = 1.0
        return x.astype(np.float32)
    x = rng.standard_normal((n, D))
    if kind == "tiny":
        x *= 1e-6
    elif kind == "large":
        x *= 1e4
    elif kind == "saturated":
        th = make_theta(D, kind)
        w = th[:D]
        target = np.where(np.arange(n) % 2 == 0, 40.0, -40.0) * np.where(np.arange(n) % 4 == 3, 20.0, 1.0)
        x = x + ((target - (x @ w + th[D])) / (w @ w))[:, None] * w[None, :]
    elif kind != "gauss":
        raise ValueError(kind)
    return x.astype(np.float32)


def make_labels(n, seed=3):
    """(n,) int64 in {0, 1} with both classes present from n = 2 on."""
    y = (np.random.default_rng(seed + n).random(n) < 0.5).astype(np.int64)
    if n >= 2:
        y[0], y[1] = 0, 1
    return y


def spoil(phi, y):
    """Copies with three invalid windows (a NaN feature, an inf feature, label 2) when n >= 8; returns
    (phi, y, number spoiled)."""
    phi, y = phi.copy(), y.copy()
    n = len(y)
    if n < 8:
        return phi, y, 0
    phi[2, phi.shape[1] // 2] = np.nan
    phi[5, 0] = np.inf
    y[n - 1] = 2
    return phi, y, 3


def _valid(phi, y):
    return np.isfinite(phi.astype(np.float64)).all(axis=1) & ((y == 0) | (y == 1))


def term_bound(phi, theta, y):
    """Sums of the absolute terms of every output entry of the fit, from the float64 reference:
    ``H_ab: sum_i w_i |phi~_ia| |phi~_ib|``, ``g_a: sum_i |p_i - y_i| |phi~_ia|``, ``loglik: sum_i |ll_i|``."""
    ok = _valid(phi, y)
    x = np.abs(np.concatenate([phi[ok].astype(np.float64), np.ones((int(ok.sum()), 1))], axis=1))
    xs = np.concatenate([phi[ok].astype(np.float64), np.ones((int(ok.sum()), 1))], axis=1)
    f = xs @ theta
    t = y[ok] == 1
    w = expit(f) * expit(-f)
    r = np.abs(expit(f) - t)
    return {"H": (x * w[:, None]).T @ x, "g": x.T @ r, "loglik": float(np.sum(np.logaddexp(0.0, np.where(t, -f, f)))),
            "n_valid": int(ok.sum())}


def gram_allowance(phi, theta, y):
    """Per entry ``(n_valid + 16) 2^-52 sum|term|``: fp64 accumulation over the windows in another order plus a few
    ulps of exp / log1p in every window's weight."""
    tb = term_bound(phi, theta, y)
    k = (tb["n_valid"] + 16) * 2.0 ** -52
    return {"H": k * tb["H"], "g": k * tb["g"], "loglik": k * tb["loglik"], "n_valid": tb["n_valid"]}


def predict_term_bound(phi, theta, chol):
    """Term sums of the prediction outputs from the float64 reference (windows with a non-finite feature: 0).

    ``mu_i = sum_c theta_c phi~_ic`` has the terms ``|theta_c phi~_ic|``.  ``v_i = sum_j psi_ij^2`` with
    ``psi_ij = sum_c phi~_ic L_cj``: an error of ``k A_ij`` in ``psi_ij`` (``A_ij = sum_c |phi~_ic L_cj|``)
    moves the square by ``2 |psi_ij| k A_ij``, and the sum of squares adds its own ``k sum_j psi_ij^2``, so the
    terms of ``v_i`` are ``2 |psi_ij| A_ij + psi_ij^2``."""
    x = phi.astype(np.float64)
    bad = ~np.isfinite(x).all(axis=1)
    x = np.where(bad[:, None], 0.0, x)
    xt = np.concatenate([x, np.ones((len(x), 1))], axis=1)
    psi = xt @ chol
    A = np.abs(xt) @ np.abs(chol)
    return {"mu": np.abs(xt) @ np.abs(theta), "v": np.sum(2.0 * np.abs(psi) * A + psi * psi, axis=1),
            "mu_ref": xt @ theta, "bad": bad}


def predict_allowance(phi, theta, chol):
    """``mu``, ``v``: ``(D + 17) 2^-52 sum|term|``; ``probit = sigmoid(mu / sqrt(1 + pi v / 8))``: ``2^-50`` plus the
    propagated allowances (|sigmoid'| <= 1/4, the denominator is >= 1, and d/dv of it is <= pi / 16);
    ``preds``: ``2^-23`` absolute (fp32 rounding of a probability plus fp64 noise in the logit)."""
    D = phi.shape[1]
    tb = predict_term_bound(phi, theta, chol)
    k = (D + 17) * 2.0 ** -52
    mu, v = k * tb["mu"], k * tb["v"]
    return {"mu": mu, "v": v, "probit": 2.0 ** -50 + 0.25 * (mu + np.abs(tb["mu_ref"]) * (np.pi / 16.0) * v),
            "preds": 2.0 ** -23, "bad": tb["bad"]}
