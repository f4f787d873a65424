"""Last-layer Laplace approximation (LLLA): a third sampler next to MC Dropout and Deep Ensembles.

One trained network, one deterministic forward pass, a Gaussian posterior over the ``Dense(1)`` head only.
With ``D = spec.final_channels``, ``phi_i`` the penultimate feature of window i (GAP of the last block after
BN on the moving statistics, dropout off; ``AlarconCNN1D.last_layer_features``), ``phi~_i = [phi_i; 1]``,
``theta = [dense kernel; dense bias]``, ``f_i = theta . phi~_i`` and ``p_i = sigmoid(f_i)``:

* fit        ``H = sum_i p_i (1 - p_i) phi~_i phi~_i^T`` (for a sigmoid head with the BCE loss the generalised
             Gauss-Newton matrix is the exact Hessian), ``g = sum_i (p_i - y_i) phi~_i``, the log-likelihood
             (from the logit, ``-softplus(-/+f)``) and the number of valid windows; a window with a non-finite
             feature or a label other than 0 / 1 is skipped and counted in ``n_total - n_valid``;
* posterior  prior ``N(0, I / lambda)`` on all D + 1 entries, precision ``P = H + lambda I``, covariance
             ``Sigma = P^-1 = L L^T`` (host float64 Cholesky of P, ``L = C^-T``).  ``theta`` is the trained head,
             not re-optimised (post-hoc Laplace); ``|g + lambda theta|`` is reported as ``map_gradient_norm``;
* evidence   ``log Z(lambda) = loglik - lambda/2 |theta|^2 + (D+1)/2 log lambda - 1/2 sum_j log(e_j + lambda)``
             with ``e_j`` the eigenvalues of H clipped at 0; ``prior_precision="auto"`` maximises it over
             ``[1e-6, 1e6]``;
* predict    ``mu_i = f_i``, ``v_i = |L^T phi~_i|^2``, ``probit_i = sigmoid(mu_i / sqrt(1 + pi v_i / 8))`` and T
             samples ``sigmoid((theta + L z_t) . phi~_i)`` with ``z = default_rng(seed).standard_normal((T, D + 1))``
             drawn on the host in float64, so the draws do not depend on the device.

All arithmetic on features is float64 on the float32 feature values.  The device work (the weighted Gram sums
of the fit set, one fp64 GEMM per prediction call) is ``ops/laplace.py`` / ``csrc/uq_laplace.hip``; the
``golden_*`` functions are float64 NumPy straight from the definitions and serve as the oracle.  A Laplace
prediction set has the shape and meaning of an ensemble's -- T models, each a draw of the head -- so every
consumer of a ``(T, N, 1)`` set takes it unchanged.
"""
from __future__ import annotations

import dataclasses
import hashlib
import json
import time
from typing import Dict, Optional, Tuple, Union

import numpy as np

PRIOR_MIN, PRIOR_MAX = 1e-6, 1e6
GRID_POINTS = 97            # log-spaced grid of the evidence search, 8 points per decade
CHUNK_WINDOWS = 65536       # windows whose features exist at a time during fit / predict


# ------------------------------------------------------------------------------------------------ evidence
def log_evidence(lam: float, eigenvalues: np.ndarray, theta: np.ndarray, loglik: float) -> float:
    e = np.clip(np.asarray(eigenvalues, np.float64), 0.0, None)
    th = np.asarray(theta, np.float64)
    return float(loglik - 0.5 * lam * (th @ th) + 0.5 * th.size * np.log(lam) - 0.5 * np.sum(np.log(e + lam)))


def optimize_prior_precision(eigenvalues, theta, loglik) -> Tuple[float, float, bool]:
    """``(lambda, log_evidence, at_bound)``: the maximiser of :func:`log_evidence` over ``[1e-6, 1e6]``.

    ``log Z`` is concave in ``log lambda`` (its derivative ``(D+1)/2 - lambda |theta|^2 / 2 - 1/2 sum_j
    lambda / (e_j + lambda)`` decreases), so the best point of a log-spaced grid brackets the maximum; a bounded
    scalar search between its neighbours refines it.  A maximiser at a bound is kept and flagged."""
    from scipy.optimize import minimize_scalar

    u = np.linspace(np.log(PRIOR_MIN), np.log(PRIOR_MAX), GRID_POINTS)
    lams = np.exp(u)
    lams[0], lams[-1] = PRIOR_MIN, PRIOR_MAX
    vals = np.array([log_evidence(l, eigenvalues, theta, loglik) for l in lams])
    k = int(np.argmax(vals))
    best_lam, best = float(lams[k]), float(vals[k])
    at_bound = k in (0, GRID_POINTS - 1)
    lo, hi = u[max(k - 1, 0)], u[min(k + 1, GRID_POINTS - 1)]
    res = minimize_scalar(lambda t: -log_evidence(float(np.exp(t)), eigenvalues, theta, loglik), bounds=(lo, hi),
                          method="bounded", options={"xatol": 1e-12})
    if res.success or np.isfinite(res.fun):
        lam_r = float(np.clip(np.exp(res.x), PRIOR_MIN, PRIOR_MAX))
        val_r = log_evidence(lam_r, eigenvalues, theta, loglik)
        if val_r > best:
            best_lam, best, at_bound = lam_r, val_r, lam_r in (PRIOR_MIN, PRIOR_MAX)
    return best_lam, best, bool(at_bound)


# ------------------------------------------------------------------------------------------------ state
def weights_hash(model) -> str:
    """SHA-256 of the model's weights (the Keras-ordered float32 arrays)."""
    h = hashlib.sha256()
    for a in model.get_weights():
        a = np.ascontiguousarray(np.asarray(a, np.float32))
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def head_theta(model) -> np.ndarray:
    """``[dense kernel; dense bias]`` (D + 1,) float64 of the model's float32 head."""
    p = model.params
    w = p["output_layer/kernel"].detach().float().cpu().numpy().reshape(-1)
    b = p["output_layer/bias"].detach().float().cpu().numpy().reshape(-1)
    return np.concatenate([w, b]).astype(np.float64)


def _factorise(H: np.ndarray, lam: float) -> np.ndarray:
    """L with ``L L^T = (H + lambda I)^-1``: ``L = C^-T`` of the Cholesky factor ``P = C C^T``."""
    from scipy.linalg import solve_triangular

    d1 = H.shape[0]
    C = np.linalg.cholesky(H + lam * np.eye(d1))
    return np.ascontiguousarray(solve_triangular(C, np.eye(d1), lower=True).T)


_ARRAYS = ("theta", "H", "g", "chol")
_SCALARS = ("loglik", "prior_precision", "log_evidence", "map_gradient_norm")


@dataclasses.dataclass
class LaplaceState:
    """The fitted posterior.  Arrays are float64 NumPy; ``chol`` is L with ``L L^T = (H + lambda I)^-1``."""
    theta: np.ndarray
    H: np.ndarray
    g: np.ndarray
    loglik: float
    n_valid: int
    n_total: int
    prior_precision: float
    prior_precision_at_bound: bool
    log_evidence: float
    map_gradient_norm: float
    chol: np.ndarray
    spec_json: str = ""
    weights_hash: str = ""

    @property
    def D(self) -> int:
        return int(self.theta.size) - 1

    def with_prior_precision(self, lam: Union[str, float]) -> "LaplaceState":
        """The posterior for another lambda (``"auto"``: evidence maximisation) from the stored sums alone."""
        return state_from_sums(self.theta, self.H, self.g, self.loglik, self.n_valid, self.n_total, lam,
                               self.spec_json, self.weights_hash)

    def scalars(self) -> Dict:
        return {"prior_precision": self.prior_precision, "prior_precision_at_bound": self.prior_precision_at_bound,
                "log_evidence": self.log_evidence, "map_gradient_norm": self.map_gradient_norm,
                "loglik": self.loglik, "n_valid": self.n_valid, "n_total": self.n_total}

    def save(self, path: str) -> str:
        """``.npz``: the float64 arrays, the float64 scalars and one JSON string; nothing is pickled."""
        meta = {"n_valid": int(self.n_valid), "n_total": int(self.n_total),
                "prior_precision_at_bound": bool(self.prior_precision_at_bound), "spec_json": self.spec_json,
                "weights_hash": self.weights_hash, "format": 1}
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, scalars=np.array([getattr(self, k) for k in _SCALARS], np.float64),
                 meta=np.array(json.dumps(meta)), **{k: np.asarray(getattr(self, k), np.float64) for k in _ARRAYS})
        return path

    @classmethod
    def load(cls, path: str) -> "LaplaceState":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"][()]))
            sc = {k: float(v) for k, v in zip(_SCALARS, z["scalars"])}
            arrs = {k: np.array(z[k], np.float64) for k in _ARRAYS}
        return cls(n_valid=int(meta["n_valid"]), n_total=int(meta["n_total"]),
                   prior_precision_at_bound=bool(meta["prior_precision_at_bound"]), spec_json=meta["spec_json"],
                   weights_hash=meta["weights_hash"], **sc, **arrs)


def state_from_sums(theta, H, g, loglik, n_valid, n_total, prior_precision: Union[str, float] = "auto",
                    spec_json: str = "", weights_hash: str = "") -> LaplaceState:
    """Prior precision (given, or the evidence maximiser), factorisation and the reported scalars."""
    theta = np.asarray(theta, np.float64)
    H = np.asarray(H, np.float64)
    g = np.asarray(g, np.float64)
    eig = np.clip(np.linalg.eigvalsh(H), 0.0, None)
    if isinstance(prior_precision, str):
        if prior_precision != "auto":
            raise ValueError("prior_precision must be 'auto' or a positive number")
        lam, logz, at_bound = optimize_prior_precision(eig, theta, float(loglik))
    else:
        lam = float(prior_precision)
        if not lam > 0.0 or not np.isfinite(lam):
            raise ValueError("prior_precision must be 'auto' or a positive number")
        logz, at_bound = log_evidence(lam, eig, theta, float(loglik)), False
    return LaplaceState(theta=theta, H=H, g=g, loglik=float(loglik), n_valid=int(n_valid), n_total=int(n_total),
                        prior_precision=lam, prior_precision_at_bound=bool(at_bound), log_evidence=float(logz),
                        map_gradient_norm=float(np.linalg.norm(g + lam * theta)), chol=_factorise(H, lam),
                        spec_json=spec_json, weights_hash=weights_hash)


# ------------------------------------------------------------------------------------------------ golden
def _phi_tilde(phi: np.ndarray) -> np.ndarray:
    x = np.asarray(phi, np.float32).astype(np.float64)
    return np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)


def golden_laplace_fit(phi, theta, y) -> Dict:
    """``{"H", "g", "loglik", "n_valid", "n_total"}`` in float64 NumPy straight from the definitions
    (``1 - p = sigmoid(-f)``, the log-likelihood from the logit)."""
    from scipy.special import expit

    xt = _phi_tilde(phi)
    th = np.asarray(theta, np.float64)
    yv = np.asarray(y).reshape(-1)
    valid = np.isfinite(xt).all(axis=1) & ((yv == 0) | (yv == 1))
    xv, t = xt[valid], (yv[valid] == 1)
    f = xv @ th
    p = expit(f)
    w = p * expit(-f)
    H = (xv * w[:, None]).T @ xv
    H = np.triu(H) + np.triu(H, 1).T
    g = xv.T @ (p - t)
    loglik = -np.sum(np.logaddexp(0.0, np.where(t, -f, f)))
    return {"H": H, "g": g, "loglik": float(loglik), "n_valid": int(valid.sum()), "n_total": int(len(yv))}


def draws(n_samples: int, d1: int, seed: int) -> np.ndarray:
    """The (T, D + 1) float64 standard normal draws of a prediction call (rows are prefix-stable in T)."""
    return np.random.default_rng(seed).standard_normal((int(n_samples), int(d1)))


def golden_laplace_predict(phi, state: LaplaceState, n_samples: int = 50, seed: int = 2025):
    """``(preds (T, n) float32, moments)`` in float64 NumPy straight from the definitions."""
    from scipy.special import expit

    xt = _phi_tilde(phi)
    bad = ~np.isfinite(xt).all(axis=1)
    xt = np.where(bad[:, None], 0.0, xt)
    z = draws(n_samples, state.theta.size, seed)
    mu = xt @ state.theta
    psi = xt @ state.chol                      # rows psi_i^T = phi~_i^T L
    v = np.sum(psi * psi, axis=1)
    thetas = state.theta[None, :] + z @ state.chol.T     # theta_t = theta + L z_t
    preds = expit(thetas @ xt.T).astype(np.float32)
    mom = {"mean_logit": mu, "logit_variance": v, "probit_prob": expit(mu / np.sqrt(1.0 + np.pi * v / 8.0)),
           "map_prob": expit(mu)}
    preds[:, bad] = np.nan
    for k in mom:
        mom[k] = np.where(bad, np.nan, mom[k])
    return preds, mom


# ------------------------------------------------------------------------------------------------ device path
def _slice(a, s: int, e: int):
    return a[s:e]


def _model_device(model):
    import torch

    return getattr(model, "device", torch.device("cpu"))


def fit_laplace(model, x_fit, y_fit, prior_precision: Union[str, float] = "auto", distributed: Optional[bool] = None,
                chunk_windows: int = CHUNK_WINDOWS) -> LaplaceState:
    """Fit the last-layer posterior of ``model`` on ``(x_fit, y_fit)``.

    Features and Gram sums are computed per chunk of ``chunk_windows`` windows, so the fit set never sits in
    memory as features.  Under an active process group (``distributed=None`` = auto) every rank fits its
    contiguous window shard and the sums travel in ONE all-reduce of one flat float64 buffer
    ``[H | g | loglik | n_valid | n_total]``.  Sums of different chunkings or shardings agree to float64
    summation order, not bitwise."""
    import torch

    from ..ops import laplace as L
    from . import distributed as DD

    n = len(x_fit)
    if len(y_fit) != n:
        raise ValueError(f"Mismatch between windows ({n}) and labels ({len(y_fit)})")
    dist_on = DD.active() if distributed is None else bool(distributed)
    s0, e0 = 0, n
    if dist_on:
        import torch.distributed as dist

        from ..parallel import dist as pdist

        s0, e0 = pdist.shard_range(n, dist.get_rank(), dist.get_world_size())
    dev = _model_device(model)
    theta = head_theta(model)
    D = theta.size - 1
    th_dev = torch.as_tensor(theta, dtype=torch.float64, device=dev)
    buf = torch.zeros(L.flat_size(D) + 1, dtype=torch.float64, device=dev)
    for s in range(s0, e0, int(chunk_windows)):
        e = min(e0, s + int(chunk_windows))
        phi = model.last_layer_features(_slice(x_fit, s, e))
        yc = _slice(y_fit, s, e)
        yc = yc if isinstance(yc, torch.Tensor) else torch.as_tensor(np.asarray(yc))
        buf[:-1] += L.gram_flat(phi, th_dev, yc.to(dev))
    buf[-1] = float(e0 - s0)
    if dist_on:
        import torch.distributed as dist

        from ..parallel import comm

        cbuf = buf.to(DD._comm_device())
        comm.run("laplace_all_reduce", cbuf, lambda: dist.all_reduce(cbuf))
        buf = cbuf
    flat = buf.cpu().numpy()
    d = L.unflatten(torch.from_numpy(flat[:-1]), D)
    spec = getattr(model, "spec", None)
    return state_from_sums(theta, d["H"].numpy().copy(), d["g"].numpy().copy(), float(d["loglik"]),
                           int(round(float(d["n_valid"]))), int(round(flat[-1])), prior_precision,
                           spec.to_json() if spec is not None else "", weights_hash(model))


def sample_matrix(state: LaplaceState, z: np.ndarray) -> np.ndarray:
    """``M = [theta_1 .. theta_T | L]`` (D + 1, T + D + 1) with ``theta_t = theta + L z_t``."""
    z = np.asarray(z, np.float64).reshape(-1, state.theta.size)
    return np.concatenate([state.theta[:, None] + state.chol @ z.T, state.chol], axis=1)


def predict_features(phi, state: LaplaceState, z: np.ndarray, eager: bool = False, return_logits: bool = False):
    """``(preds (T, n), mu, v, probit)`` torch tensors on ``phi``'s device for explicit draws ``z`` (T, D + 1):
    the entry point below :func:`laplace_predict` (features in, no model).  ``eager`` forces the torch
    float64 path, which can return the sample logits instead of the float32 probabilities."""
    import torch

    from ..ops import laplace as L

    z = np.asarray(z, np.float64).reshape(-1, state.theta.size)
    M = torch.as_tensor(sample_matrix(state, z), dtype=torch.float64, device=phi.device)
    th = torch.as_tensor(state.theta, dtype=torch.float64, device=phi.device)
    if eager or return_logits:
        return L.predict_eager(phi, M, th, z.shape[0], return_logits=return_logits)
    return L.predict(phi, M, th, z.shape[0])


def check_state(model, state: LaplaceState) -> None:
    if state.weights_hash and state.weights_hash != weights_hash(model):
        raise ValueError("this LaplaceState was fitted for a model with other weights (weight hash mismatch); "
                         "refit with fit_laplace")
    if state.D != model.spec.final_channels:
        raise ValueError(f"the state has D = {state.D}, the model {model.spec.final_channels} final channels")


def laplace_predict(model, state: LaplaceState, x, n_samples: int = 50, seed: int = 2025, as_numpy: bool = True,
                    return_moments: bool = False, chunk_windows: int = CHUNK_WINDOWS):
    """Last-layer Laplace predictions (n_samples, N, 1) float32, the shape ``mc_dropout_predict`` returns.

    One deterministic forward pass yields the features; sample t is the head ``theta + L z_t``.  With
    ``return_moments`` also ``{"mean_logit", "logit_variance", "probit_prob", "map_prob"}`` (N,) float64.
    A window with a non-finite feature is NaN in every output.  Refuses a state fitted for other weights."""
    import torch

    start = time.time()
    check_state(model, state)
    T = int(n_samples)
    if T < 0:
        raise ValueError("n_samples must be >= 0")
    z = draws(T, state.theta.size, seed)
    n = len(x)
    dev = _model_device(model)
    preds = torch.empty(T, n, dtype=torch.float32, device=dev)
    mom = torch.empty(3, n, dtype=torch.float64, device=dev)
    for s in range(0, n, int(chunk_windows)):
        e = min(n, s + int(chunk_windows))
        phi = model.last_layer_features(_slice(x, s, e))
        p, mu, v, pb = predict_features(phi, state, z)
        preds[:, s:e] = p
        mom[0, s:e], mom[1, s:e], mom[2, s:e] = mu, v, pb
    out = preds.unsqueeze(-1)
    moments = {"mean_logit": mom[0], "logit_variance": mom[1], "probit_prob": mom[2], "map_prob": torch.sigmoid(mom[0])}
    if as_numpy:
        out = out.cpu().numpy()
        moments = {k: t.cpu().numpy() for k, t in moments.items()}
    print(f"Last-layer Laplace completed in {time.time() - start:.1f}s ({T} samples)")
    return (out, moments) if return_moments else out
