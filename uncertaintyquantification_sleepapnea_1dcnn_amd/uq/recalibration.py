"""Post-hoc recalibration of a prediction set: temperature, Platt and beta calibration that keep ``(T, N, 1)``.

One monotone map is applied to every pass or member and chosen so that the *pooled* probability is calibrated
(the joint calibration of Rahaman and Thiery, 2021).  With ``p_c = clip(p, 1e-7, 1 - 1e-7)``, ``l1 = log p_c`` and
``l0 = log1p(-p_c)`` the three-parameter family of beta calibration (Kull et al., 2017) covers all methods:

    ``q_t = sigmoid(a l1_t - b l0_t + c)``

| method          | free parameters | constraint                   |
|-----------------|-----------------|------------------------------|
| ``temperature`` | 1               | ``a = b = 1 / tau``, ``c = 0`` |
| ``platt``       | 2               | ``a = b``, ``c`` free          |
| ``beta``        | 3               | ``a, b, c`` free             |

A beta fit with ``a < 0`` or ``b < 0`` would not be monotone: it is refitted with that parameter at 0
(``constrained``).

``objective="joint"`` minimises ``-sum_n log p(y_n | mean_t q_tn)``; ``"member"`` the mean over t of each pass's own
NLL (plain logistic regression on T N points).  The fit is a damped Newton iteration on the host; the loss,
gradient and Hessian of every trial step of one iteration come from ONE device launch over the whole ``(T, N)``
array (``ops/recal.py`` / ``csrc/uq_recal.hip``), in ``theta = (a, b, c)``; the host applies the linear
reparametrisation ``theta = J phi``.  A cross-fit iterates all folds together from the same launches: the kernel
keeps the sums per fold, fold f trains on the sum of the other folds' slots.

The ``golden_*`` functions are float64 NumPy / SciPy straight from the definitions: the oracle and the timing
baseline.  A recalibrated set is a prediction set again, so every analysis takes it unchanged.
"""
from __future__ import annotations

import dataclasses
import json
import os
import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import calibration as C
from . import metrics as M

METHODS = ("temperature", "platt", "beta")
OBJECTIVES = ("joint", "member")
EPS = 1e-7
DAMPINGS = (0.0, 1e-3, 1e-1, 10.0)   # Levenberg dampings, times the mean diagonal of the Hessian
STEP_LENGTHS = (1.0, 0.25)
MAX_ITER = 50
GRAD_TOL = 1e-8                      # stop at |g| / n_valid <= GRAD_TOL
LOSS_NOISE = 1e-12                   # relative rounding floor of a summed loss: below it a trial is accepted only
                                     # if it at least halves the gradient norm
THETA_MAX = 1e3                      # beyond: the data are (nearly) separable, the scale runs to infinity
SEPARABLE_NLL = 1e-6                 # a fitted mean NLL below this: every window is classified with certainty
IDENTITY = np.array([1.0, 1.0, 0.0])
METRICS = ("ece", "mce", "brier", "nll")
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _torch():
    import torch

    return torch


def basis(method: str, fixed: Sequence[str] = ()) -> np.ndarray:
    """J (3, k) with ``theta = J phi``; ``fixed`` names the beta parameters (``"a"``, ``"b"``) held at 0."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    if method == "temperature":
        return np.array([[1.0], [1.0], [0.0]])
    if method == "platt":
        return np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    keep = [i for i, name in enumerate("abc") if name not in fixed]
    return np.eye(3)[:, keep]


def _start(J: np.ndarray) -> np.ndarray:
    """phi of the identity map (least squares: exact whenever the identity is in the family)."""
    return np.linalg.lstsq(J, IDENTITY, rcond=None)[0]


def unpack_sums(row: np.ndarray) -> Tuple[float, np.ndarray, np.ndarray]:
    """(12,) -> loss, g (3,), H (3, 3)."""
    H = np.zeros((3, 3))
    for k, (i, j) in enumerate(_PAIRS):
        H[i, j] = H[j, i] = row[6 + k]
    return float(row[2]), np.array(row[3:6], np.float64), H


# ===================== Golden float64 NumPy / SciPy =====================
def _golden_planes(probs):
    p = np.asarray(probs, np.float32).astype(np.float64)
    if p.ndim == 3 and p.shape[-1] == 1:
        p = p[..., 0]
    if p.ndim == 1:
        p = p[None]
    fin = np.isfinite(p)
    pc = np.clip(np.where(fin, p, 0.5), EPS, 1 - EPS)
    return np.log(pc), np.log1p(-pc), fin


def golden_sums(probs, y, fold, thetas, n_folds: int = 1, objective: str = "joint") -> np.ndarray:
    """(F, Q, 12) float64 of ``ops.recal.sums`` straight from the definitions (``1 - q = sigmoid(-u)``)."""
    from scipy.special import expit

    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}")
    l1, l0, fin = _golden_planes(probs)
    T, n = l1.shape
    yv = np.asarray(y).reshape(-1)
    fc = np.zeros(n, np.int64) if fold is None or len(fold) == 0 else np.asarray(fold).astype(np.int64)
    valid = fin.all(axis=0) & ((yv == 0) | (yv == 1)) & (fc >= 0) & (fc < n_folds)
    y1 = yv == 1
    f = np.stack([l1, -l0, np.ones_like(l1)])                  # (3, T, n)
    thetas = np.asarray(thetas, np.float64).reshape(-1, 3)
    out = np.zeros((n_folds, len(thetas), 12))
    for qi, th in enumerate(thetas):
        u = np.tensordot(th, f, axes=1)                         # (T, n)
        q, o = expit(u), expit(-u)
        s = q * o
        if objective == "joint":
            pbar, obar = q.mean(axis=0), o.mean(axis=0)
            hit = np.where(y1, pbar, obar)
            with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                loss = -np.log(hit)
                r = np.where(y1, -1.0, 1.0) / hit
                gv = (s[None] * f).mean(axis=1)                 # (3, n)
                G = np.einsum("tn,itn,jtn->ijn", s * (1 - 2 * q), f, f) / T
                g = r * gv
                H = r * r * gv[:, None] * gv[None] + r * G
        else:
            loss = np.where(y1, np.logaddexp(0.0, -u), np.logaddexp(0.0, u)).mean(axis=0)
            g = ((q - y1) * f).mean(axis=1)
            H = np.einsum("tn,itn,jtn->ijn", s, f, f) / T
        cols = np.stack([np.ones(n), y1.astype(np.float64), loss, g[0], g[1], g[2]] + [H[i, j] for i, j in _PAIRS])
        for fi in range(n_folds):
            m = valid & (fc == fi)
            out[fi, qi] = cols[:, m].sum(axis=1)
    return out


def golden_fit(probs, y, method: str = "temperature", objective: str = "joint", fixed: Sequence[str] = ()) -> Dict:
    """The minimiser by ``scipy.optimize.minimize`` (BFGS on the mean loss, analytic gradient): ``theta``, ``phi``,
    ``nll`` (mean over the valid windows), ``H`` (the Hessian of the summed loss in phi at the optimum) and
    ``n_valid``."""
    from scipy.optimize import minimize

    J = basis(method, fixed)

    def at(phi):
        row = golden_sums(probs, y, None, (J @ phi)[None], 1, objective)[0, 0]
        loss, g, H = unpack_sums(row)
        return row[0], loss, J.T @ g, J.T @ H @ J

    nv = at(_start(J))[0]

    def fun(phi):
        _, loss, g, _ = at(phi)
        return loss / nv, g / nv

    res = minimize(fun, _start(J), jac=True, method="BFGS", options={"gtol": 1e-11, "maxiter": 500})
    phi = res.x
    for _ in range(2):  # BFGS stops at its line search's precision: two Newton steps on the analytic Hessian
        _, _, g, H = at(phi)
        step = np.linalg.solve(H, g)
        if np.all(np.isfinite(step)) and at(phi - step)[1] <= at(phi)[1]:
            phi = phi - step
    _, loss, g, H = at(phi)
    return {"theta": J @ phi, "phi": phi, "nll": loss / nv, "H": H, "g": g, "n_valid": int(round(nv))}


def golden_apply(probs, theta, fold=None) -> np.ndarray:
    """(T, n) float32 of the map (``theta`` (3,) or per fold (F, 3)) straight from the definition."""
    from scipy.special import expit

    l1, l0, fin = _golden_planes(probs)
    th = np.asarray(theta, np.float64).reshape(-1, 3)
    n = l1.shape[1]
    fc = np.zeros(n, np.int64) if fold is None or len(fold) == 0 else np.asarray(fold).astype(np.int64)
    ok = (fc >= 0) & (fc < len(th))
    tw = th[np.where(ok, fc, 0)]
    q = expit(tw[:, 0] * l1 - tw[:, 1] * l0 + tw[:, 2]).astype(np.float32)
    q[~(fin & ok[None])] = np.nan
    return q


# ===================== Newton on the device sums =====================
@dataclasses.dataclass
class _Fit:
    """One fit of a (possibly batched) Newton iteration."""
    J: np.ndarray
    phi: np.ndarray
    row: Optional[np.ndarray] = None      # the training sums (12,) at phi
    held: Optional[np.ndarray] = None     # the held-out sums (12,) at phi (cross-fit)
    row0: Optional[np.ndarray] = None
    held0: Optional[np.ndarray] = None
    n_iter: int = 0
    done: bool = False
    converged: bool = False

    @property
    def theta(self) -> np.ndarray:
        return self.J @ self.phi

    def grad(self) -> np.ndarray:
        return self.J.T @ unpack_sums(self.row)[1]

    def grad_norm(self) -> float:
        return float(np.linalg.norm(self.grad()) / max(self.row[0], 1.0))


def _trials(fit: _Fit) -> np.ndarray:
    """(8, k) trial points: Levenberg dampings x step lengths (a singular system gives NaN = rejected)."""
    _, g, H = unpack_sums(fit.row)
    gp, Hp = fit.J.T @ g, fit.J.T @ H @ fit.J
    mu = float(np.mean(np.abs(np.diag(Hp)))) or 1.0
    out = []
    for lam in DAMPINGS:
        try:
            step = -np.linalg.solve(Hp + lam * mu * np.eye(len(gp)), gp)
        except np.linalg.LinAlgError:
            step = np.full(len(gp), np.nan)
        out += [fit.phi + s * step for s in STEP_LENGTHS]
    return np.array(out)


def _run_newton(sum_fn: Callable[[np.ndarray], np.ndarray], fits: List[_Fit],
                split: Callable[[int, np.ndarray], Tuple[np.ndarray, np.ndarray]], max_q: int = 64) -> None:
    """Damped Newton for all ``fits`` together.  ``sum_fn(thetas (Q, 3)) -> (F, Q, 12)`` (already summed over the
    ranks); ``split(i, (F, 12)) -> (training, held-out)`` sums of fit i."""

    def evaluate(points: List[np.ndarray]) -> np.ndarray:
        th = np.array(points).reshape(-1, 3)
        th = np.where(np.isfinite(th), th, 0.0)
        return np.concatenate([sum_fn(th[s:s + max_q]) for s in range(0, len(th), max_q)], axis=1)

    out = evaluate([fits[0].theta]) if all(np.array_equal(f.theta, fits[0].theta) for f in fits) else None
    for i, f in enumerate(fits):
        o = out[:, 0] if out is not None else evaluate([f.theta])[:, 0]
        f.row, f.held = split(i, o)
        f.row0, f.held0 = f.row, f.held
    for f in fits:
        nv, ny = f.row[0], f.row[1]
        if nv < 1 or ny == 0 or ny == nv:
            raise ValueError("the fit set needs valid windows of both classes")
        if f.grad_norm() <= GRAD_TOL:
            f.done = f.converged = True
    for _ in range(MAX_ITER):
        active = [i for i, f in enumerate(fits) if not f.done]
        if not active:
            break
        trials = [_trials(fits[i]) for i in active]
        nt = len(trials[0])
        out = evaluate([fits[i].J @ ph if np.all(np.isfinite(ph)) else np.full(3, np.nan)
                        for i, tr in zip(active, trials) for ph in tr])
        for k, (i, tr) in enumerate(zip(active, trials)):
            f = fits[i]
            f.n_iter += 1
            best, best_loss = None, f.row[2]
            flat, flat_grad = None, 0.5 * f.grad_norm()
            for j in range(nt):
                if not np.all(np.isfinite(tr[j])):
                    continue
                row, held = split(i, out[:, k * nt + j])
                if not np.all(np.isfinite(row)):
                    continue
                if row[2] < best_loss:
                    best, best_loss = (tr[j], row, held), row[2]
                elif row[2] <= f.row[2] * (1.0 + LOSS_NOISE):
                    gn = float(np.linalg.norm(f.J.T @ row[3:6]) / max(row[0], 1.0))
                    if gn < flat_grad:
                        flat, flat_grad = (tr[j], row, held), gn
            if best is None:          # at the rounding floor of the summed loss the gradient still tells steps apart
                best = flat
            if best is None:          # no trial lowers the loss
                f.done = f.converged = True
                continue
            f.phi, f.row, f.held = best
            if np.max(np.abs(f.theta)) > THETA_MAX:
                f.done, f.converged = True, False
            elif f.grad_norm() <= GRAD_TOL:
                f.done = f.converged = True
    for f in fits:
        if f.converged and f.row[2] / f.row[0] < SEPARABLE_NLL:
            f.converged = False


@dataclasses.dataclass
class Recalibrator:
    """A fitted map.  ``nll_before`` / ``nll_after`` are means over the ``n_valid`` fit windows of the objective
    at the identity and at ``theta``; ``grad_norm`` is ``|g| / n_valid`` in the free parameters; ``constrained``
    names the beta parameters that were refitted at 0."""
    method: str
    objective: str
    theta: np.ndarray
    temperature: Optional[float]
    nll_before: float
    nll_after: float
    n_valid: int
    n_iter: int
    grad_norm: float
    converged: bool
    constrained: Tuple[str, ...] = ()

    def apply(self, predictions):
        """The calibrated set, ``(T, N, 1)`` float32 of the input's kind (NumPy, or a torch tensor on its device)."""
        return _apply(predictions, np.asarray(self.theta, np.float64)[None], None)

    def scalars(self) -> Dict:
        return {"method": self.method, "objective": self.objective, "temperature": self.temperature,
                "nll_before": self.nll_before, "nll_after": self.nll_after, "n_valid": int(self.n_valid),
                "n_iter": int(self.n_iter), "grad_norm": self.grad_norm, "converged": bool(self.converged),
                "constrained": list(self.constrained)}

    def save(self, path: str) -> str:
        """``.npz``: the float64 theta and one JSON string; nothing is pickled."""
        if not path.endswith(".npz"):
            path += ".npz"
        meta = dict(self.scalars(), format=1)
        np.savez(path, theta=np.asarray(self.theta, np.float64), meta=np.array(json.dumps(meta)))
        return path

    @classmethod
    def load(cls, path: str) -> "Recalibrator":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"][()]))
            theta = np.array(z["theta"], np.float64)
        meta.pop("format", None)
        meta["constrained"] = tuple(meta["constrained"])
        return cls(theta=theta, **meta)


def _on_device(predictions):
    """(T, N) float32 torch tensor on the device the work runs on (the GPU when there is one)."""
    p2 = C._as_tensor_2d(predictions)
    if not p2.is_cuda and C._use_device(predictions):
        p2 = p2.to("cuda")
    return p2.contiguous()


def _apply(predictions, thetas: np.ndarray, fold):
    torch = _torch()
    from ..ops import recal

    p2 = _on_device(predictions)
    fd = None if fold is None else torch.as_tensor(np.asarray(fold, np.int32), device=p2.device)
    out = recal.apply(p2, fd, torch.as_tensor(thetas, dtype=torch.float64, device=p2.device))[..., None]
    if isinstance(predictions, torch.Tensor):
        return out.to(predictions.device)
    return out.cpu().numpy()


def _labels_tensor(y, device):
    torch = _torch()
    yy = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
    return yy.reshape(-1).to(device)


def _sum_fn(p2, y, fold, n_folds: int, objective: str, dist_on: bool):
    """``thetas (Q, 3) numpy -> (F, Q, 12) numpy``: one launch, and one all-reduce under a process group."""
    torch = _torch()
    from ..ops import recal

    def fn(thetas: np.ndarray) -> np.ndarray:
        th = torch.as_tensor(np.ascontiguousarray(thetas), dtype=torch.float64, device=p2.device)
        if p2.shape[1]:
            out = recal.sums(p2, y, fold, th, n_folds, objective)
        else:
            out = torch.zeros(n_folds, len(thetas), recal.COLS, dtype=torch.float64, device=p2.device)
        if dist_on:
            import torch.distributed as dist

            from ..parallel import comm
            from . import distributed as DD

            cbuf = out.to(DD._comm_device())
            comm.run("recal_all_reduce", cbuf, lambda: dist.all_reduce(cbuf))
            out = cbuf
        return out.cpu().numpy()

    return fn


def _result(f: _Fit, method: str, objective: str, constrained: Tuple[str, ...]) -> Recalibrator:
    theta = f.theta
    nv = f.row[0]
    return Recalibrator(method=method, objective=objective, theta=theta,
                        temperature=float(1.0 / theta[0]) if method == "temperature" else None,
                        nll_before=float(f.row0[2] / nv), nll_after=float(f.row[2] / nv), n_valid=int(round(nv)),
                        n_iter=int(f.n_iter), grad_norm=f.grad_norm(), converged=bool(f.converged),
                        constrained=tuple(constrained))


def _warn_unconverged(what: str, f: _Fit) -> None:
    warnings.warn(f"{what}: the fit did not converge (max |theta| = {np.max(np.abs(f.theta)):.3g}, mean NLL "
                  f"{f.row[2] / f.row[0]:.3g} after {f.n_iter} iterations); separable data drive the scale to "
                  "infinity", RuntimeWarning, stacklevel=3)


def _check_args(method: str, objective: str) -> None:
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}")


def _fit_with_refit(sum_fn, method: str, n_fits: int, split) -> Tuple[List[_Fit], List[Tuple[str, ...]]]:
    """All fits, then the beta fits with a negative ``a`` or ``b`` again with that parameter at 0."""
    J = basis(method)
    fits = [_Fit(J=J, phi=_start(J)) for _ in range(n_fits)]
    _run_newton(sum_fn, fits, split)
    fixed: List[Tuple[str, ...]] = [() for _ in fits]
    if method == "beta":
        for _ in range(2):  # fixing one parameter can push the other below 0
            redo = [i for i, f in enumerate(fits) if f.theta[0] < 0 or f.theta[1] < 0]
            if not redo:
                break
            for i in redo:
                th = fits[i].theta
                fixed[i] = tuple(sorted(set(fixed[i]) | {nm for nm, v in (("a", th[0]), ("b", th[1])) if v < 0}))
                Ji = basis("beta", fixed[i])
                new = _Fit(J=Ji, phi=_start(Ji))
                _run_newton(sum_fn, [new], lambda _k, o, i=i: split(i, o))
                # "before" stays the identity map's loss
                new.row0, new.held0, new.n_iter = fits[i].row0, fits[i].held0, fits[i].n_iter + new.n_iter
                fits[i] = new
    return fits, fixed


def fit_recalibration(predictions, y, method: str = "temperature", objective: str = "joint",
                      distributed: Optional[bool] = None) -> Recalibrator:
    """Fit one map on ``(predictions, y)``: damped Newton from the identity, one device launch per iteration.

    Stops at ``|g| / n_valid <= 1e-8``, when no trial step lowers the loss (within 1e-12 relative of it, the
    rounding floor of the summed loss, a trial that halves the gradient norm still counts), or after 50 iterations (then
    ``converged`` is False, as it is when ``max |theta| > 1e3`` or the fitted mean NLL is below 1e-6: separable
    data drive the scale to infinity; a warning says so).  A fit set with one class raises ``ValueError``.  Under
    an active process group (``distributed=None`` = auto) every rank sums its contiguous window shard and the
    ``(F, Q, 12)`` array travels in one all-reduce per iteration."""
    from . import distributed as DD

    _check_args(method, objective)
    p2 = _on_device(predictions)
    yy = _labels_tensor(y, p2.device)
    if yy.numel() != p2.shape[1]:
        raise ValueError(f"Mismatch between prediction samples ({p2.shape[1]}) and label samples ({yy.numel()})")
    dist_on = DD.active() if distributed is None else bool(distributed)
    if dist_on:
        import torch.distributed as dist

        from ..parallel import dist as pdist

        s, e = pdist.shard_range(p2.shape[1], dist.get_rank(), dist.get_world_size())
        p2, yy = p2[:, s:e].contiguous(), yy[s:e]
    fn = _sum_fn(p2, yy, None, 1, objective, dist_on)
    fits, fixed = _fit_with_refit(fn, method, 1, lambda _i, o: (o[0], o[0]))
    if not fits[0].converged:
        _warn_unconverged("fit_recalibration", fits[0])
    return _result(fits[0], method, objective, fixed[0])


def assign_folds(groups, n_folds: int, seed: int = 2025, n: Optional[int] = None) -> np.ndarray:
    """(n,) int32 fold codes that never split a group: the sorted unique ids are permuted with
    ``numpy.random.default_rng(seed).permutation(P)`` and the id of permuted rank r goes to fold ``r % n_folds``.
    ``groups=None``: every one of the ``n`` windows is its own group."""
    if groups is None:
        if n is None:
            raise ValueError("assign_folds needs groups or n")
        P, inverse = int(n), np.arange(int(n))
    else:
        ids, inverse = np.unique(np.asarray(groups).reshape(-1), return_inverse=True)
        P = len(ids)
    if not 2 <= int(n_folds) <= P:
        raise ValueError("n_folds must be in 2..number of groups")
    perm = np.random.default_rng(seed).permutation(P)
    fold_of = np.empty(P, np.int32)
    fold_of[perm] = np.arange(P, dtype=np.int32) % int(n_folds)
    return fold_of[inverse.reshape(-1)]


def cross_recalibrate(predictions, y, groups=None, n_folds: int = 5, method: str = "temperature",
                      objective: str = "joint", seed: int = 2025, fold=None):
    """``(calibrated predictions, info)``: every window is mapped by the fit on the other folds.

    All folds iterate together, one launch per Newton iteration (the kernel keeps the sums per fold).  ``info``:
    ``fold`` (n,), ``theta`` (F, 3), ``n_iter``, ``converged``, ``constrained`` per fold and the held-out mean NLL
    ``nll_before`` / ``nll_after`` per fold and overall.  A fold whose complement lacks a class raises
    ``ValueError``.  ``fold`` overrides :func:`assign_folds` with given codes."""
    from ..ops import recal

    torch = _torch()
    _check_args(method, objective)
    F = int(n_folds)
    if not 2 <= F <= recal.MAX_F:
        raise ValueError(f"n_folds must be in 2..{recal.MAX_F}")
    p2 = _on_device(predictions)
    n = p2.shape[1]
    yy = _labels_tensor(y, p2.device)
    if yy.numel() != n:
        raise ValueError(f"Mismatch between prediction samples ({n}) and label samples ({yy.numel()})")
    codes = assign_folds(groups, F, seed, n) if fold is None else np.asarray(fold, np.int32).reshape(-1)
    if len(codes) != n:
        raise ValueError("one fold code (or group id) per window")
    fd = torch.as_tensor(codes, dtype=torch.int32, device=p2.device)
    fn = _sum_fn(p2, yy, fd, F, objective, False)

    def split(i, o):
        return np.delete(o, i, axis=0).sum(axis=0), o[i]

    fits, fixed = _fit_with_refit(fn, method, F, split)
    for i, f in enumerate(fits):
        if not f.converged:
            _warn_unconverged(f"cross_recalibrate fold {i}", f)
    thetas = np.array([f.theta for f in fits])
    held0 = np.array([f.held0 for f in fits])
    held = np.array([f.held for f in fits])
    nz = np.maximum(held[:, 0], 1.0)
    info = {"fold": codes, "theta": thetas, "method": method, "objective": objective,
            "n_iter": [int(f.n_iter) for f in fits], "converged": [bool(f.converged) for f in fits],
            "constrained": [tuple(c) for c in fixed], "n_valid": held[:, 0].astype(np.int64),
            "fold_nll_before": held0[:, 2] / nz, "fold_nll_after": held[:, 2] / nz,
            "nll_before": float(held0[:, 2].sum() / max(held[:, 0].sum(), 1.0)),
            "nll_after": float(held[:, 2].sum() / max(held[:, 0].sum(), 1.0))}
    return _apply(predictions, thetas, codes), info


# ===================== Evaluation =====================
def evaluate_recalibration(predictions, y, evaluation_label: str = "Recalibration", fit_predictions=None, fit_y=None,
                           patient_ids=None, n_folds: int = 5, method: str = "temperature", objective: str = "joint",
                           n_bootstrap: int = 100, random_state: Optional[int] = None, parity: bool = True,
                           n_bins: int = 15, output_plot_dir: str = "./uq_plots", make_plots: bool = True,
                           seed: int = 2025, return_details: bool = False):
    """Calibration before and after recalibration as one flat dictionary.

    With a fit set (``fit_predictions``, ``fit_y``) the map is fitted there and applied to ``predictions``;
    otherwise ``predictions`` are cross-fitted in ``n_folds`` folds that never split a patient
    (``patient_ids=None``: folds of windows).  Per metric m of ``ece``, ``mce``, ``brier``, ``nll``:
    ``{m}_before``, ``{m}_after``, ``{m}_diff`` (after - before) and, on the SAME resamples before and after,
    ``{m}_diff_mean``, ``{m}_diff_ci_lower``, ``{m}_diff_ci_upper`` and ``{m}_share_improved`` (the share of the
    replicates with after < before).  The parameters follow: ``theta_a/b/c`` (and ``temperature``) of the single
    fit, or ``theta_a/b/c_fold{f}`` of the cross-fit, ``fit_nll_before`` / ``fit_nll_after`` (the objective on the
    fit windows, held out in a cross-fit), ``converged``.  ``return_details``: also the calibrated set, the
    replicate-wise differences and the :class:`Recalibrator` or the cross-fit ``info``."""
    from ..ops import calib

    torch = _torch()
    _check_args(method, objective)
    final: Dict[str, float] = {"method": method, "objective": objective}
    if (fit_predictions is None) != (fit_y is None):
        raise ValueError("fit_predictions and fit_y go together")
    if fit_predictions is not None:
        fitted = fit_recalibration(fit_predictions, fit_y, method, objective)
        after = fitted.apply(predictions)
        for name, v in zip("abc", fitted.theta):
            final[f"theta_{name}"] = float(v)
        if fitted.temperature is not None:
            final["temperature"] = fitted.temperature
        final.update(fit_nll_before=fitted.nll_before, fit_nll_after=fitted.nll_after, n_iter=fitted.n_iter,
                     converged=bool(fitted.converged))
    else:
        after, fitted = cross_recalibrate(predictions, y, patient_ids, n_folds, method, objective, seed)
        for fi, th in enumerate(fitted["theta"]):
            for name, v in zip("abc", th):
                final[f"theta_{name}_fold{fi}"] = float(v)
        final.update(fit_nll_before=fitted["nll_before"], fit_nll_after=fitted["nll_after"],
                     n_iter=int(max(fitted["n_iter"])), converged=bool(all(fitted["converged"])))
    dev = "cuda" if C._use_device(predictions) else None
    yy = C._labels(y)
    pts, boots = [], []
    idx = None
    for k, pred in enumerate((predictions, after)):
        p, s = C.per_window(pred, "pred_variance", dev)
        n = p.numel()
        if len(yy) != n:
            raise ValueError(f"Mismatch between prediction samples ({n}) and label samples ({len(yy)})")
        rec = C._records(p, s, yy, np.zeros(0, np.float32), n_bins)
        pts.append(C._point(rec, n_bins, 0))
        if n_bootstrap:
            if parity and idx is None:
                idx = torch.as_tensor(M.parity_bootstrap_indices(n, n_bootstrap, random_state).astype(np.int32),
                                      device=rec.device)
            sums = calib.bootstrap_sums(rec, n_bootstrap, n_bins, 0, idx=idx,
                                        seed=0 if random_state is None else random_state)
            boots.append(calib.finalize(sums, n, n_bins, 0))
    reps: Dict[str, np.ndarray] = {}
    for m in METRICS:
        b, a = float(pts[0][m]), float(pts[1][m])
        final[f"{m}_before"], final[f"{m}_after"], final[f"{m}_diff"] = b, a, a - b
        if n_bootstrap:
            d = boots[1][m] - boots[0][m]
            reps[m] = d
            final[f"{m}_diff_mean"], final[f"{m}_diff_ci_lower"], final[f"{m}_diff_ci_upper"] = C._ci(d)
            ok = ~np.isnan(d)
            final[f"{m}_share_improved"] = float(np.mean(d[ok] < 0)) if ok.any() else float("nan")
    if make_plots:
        plot_reliability_pair(pts[0], pts[1], evaluation_label, output_plot_dir)
    if return_details:
        return final, {"calibrated": after, "replicates": reps, "fit": fitted, "idx": idx}
    return final


def plot_reliability_pair(before: Dict, after: Dict, uq_name: str, output_dir: str = "./uq_plots"):
    """Reliability diagram with two curves: before and after recalibration."""
    plt = C.plt
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(6, 6))
    plt.plot([0, 1], [0, 1], "k--", alpha=0.5, label="Perfect calibration")
    for pt, name, style in ((before, "before", "o-"), (after, "after", "s-")):
        ok = pt["bin_count"] > 0
        plt.plot(pt["bin_confidence"][ok], pt["bin_frequency"][ok], style, label=f"{name}: ECE {float(pt['ece']):.4f}")
    plt.xlabel("Mean predicted probability")
    plt.ylabel("Observed frequency of apnea/hypopnea")
    plt.title(f"Reliability before / after recalibration - {uq_name}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"reliability_recalibrated_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)
