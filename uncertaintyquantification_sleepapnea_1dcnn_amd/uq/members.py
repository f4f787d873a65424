"""Ensemble composition from one prediction set: how different the members are, which of them carry the
ensemble, and whether k chosen members would do what all T do.

The other analyses treat a ``(T, N, 1)`` set as T exchangeable draws.  The members of a Deep Ensemble are
trained networks with names and files, each costing one forward pass per window for ever:

* :func:`member_table` scores every member on its own and by what the ensemble loses without it;
* :func:`member_diversity` gives the pairwise disagreement, double-fault, Q statistic, error correlation,
  Cohen's kappa and residual correlation, their means over the pairs, the Kohavi-Wolpert variance and the
  Krogh-Vedelsby decomposition ``ensemble Brier = mean member Brier - ambiguity``;
* :func:`select_members` is greedy forward selection (Caruana et al. 2004), cross-fitted by patient when asked:
  selected on some patients, scored on the others;
* :func:`evaluate_members` puts the greedy curve next to the first-k and the random-k curves and reports the
  count from which on the greedy sub-ensemble stays within a tolerance of all T.

The sums behind them come from ``ops/members.py`` (``csrc/uq_members.hip`` on CUDA predictions, the eager
emulation otherwise); they are integers, so every selection step is decided on integers and is the same for
any grid and any sharding.  ``golden_member_pairs``, ``golden_mix`` and ``golden_select`` are float64 NumPy
written from the definitions: the test oracles and the timing baseline.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import pandas as pd

from . import calibration as C
from . import metrics as M
from .convergence import default_counts, subset_orders

plt = C.plt

LOSSES = ("nll", "brier")
DEFAULT_TOLERANCE = 1e-3   # absolute, in the loss's own unit (nats per window for nll, squared probability for brier)
MEANS = ("disagreement", "kappa", "q_statistic", "double_fault", "error_correlation", "residual_correlation")


def _torch():
    import torch

    return torch


def _ops():
    from ..ops import members as MB

    return MB


# ===================== Golden float64 NumPy implementations =====================
def _golden_inputs(predictions, y):
    p = M.as_2d(np.asarray(predictions)).astype(np.float32)
    yy = np.asarray(y).reshape(-1) != 0
    if p.shape[1] != len(yy):
        raise ValueError(f"Mismatch between prediction samples ({p.shape[1]}) and label samples ({len(yy)})")
    ok = np.all(np.isfinite(p), axis=0)
    return p.astype(np.float64), yy, ok


def golden_member_pairs(predictions, y):
    """The (T, T, 3) int64 pair table and the (n_valid, n_y1) header, pair by pair from the definitions."""
    p, yy, ok = _golden_inputs(predictions, y)
    p, yy = p[:, ok], yy[ok]
    t_count = p.shape[0]
    r = p - yy.astype(np.float64)
    c = (p > 0.5) == yy
    table = np.zeros((t_count, t_count, 3), np.int64)
    for a in range(t_count):
        for b in range(t_count):
            both = c[a] & c[b]
            table[a, b, 0] = np.sum(both & ~yy)
            table[a, b, 1] = np.sum(both & yy)
            table[a, b, 2] = np.rint(r[a] * r[b] * float(2 ** 40)).astype(np.int64).sum()
    return table, np.array([p.shape[1], int(yy.sum())], np.int64)


def golden_mix(predictions, y, counts, fold=None, n_folds: int = 1) -> np.ndarray:
    """(F, Q, 7) int64: per fold and row of counts the sums n_valid, n_y1, rint(nll 2^36), rint((m - y)^2 2^40),
    correct, true_pos, pred_pos of the mixture m = (sum_t c_t p_t) / k, row by row from the definitions."""
    p, yy, ok = _golden_inputs(predictions, y)
    counts = np.asarray(counts, np.int64).reshape(-1, p.shape[0])
    fo = np.zeros(len(yy), np.int64) if fold is None else np.asarray(fold, np.int64).reshape(-1)
    p, yy, fo = p[:, ok], yy[ok], fo[ok]
    yd = yy.astype(np.float64)
    out = np.zeros((int(n_folds), len(counts), 7), np.int64)
    for q, c in enumerate(counts):
        s = np.zeros(p.shape[1])
        for t in range(p.shape[0]):
            s = s + float(c[t]) * p[t]
        k = float(c.sum())
        m = s / k
        lab = 2.0 * s > k
        nll = -np.log(np.clip(np.where(yy, m, 1.0 - m), 1e-7, 1 - 1e-7))
        cols = [np.ones(len(yy), np.int64), yy.astype(np.int64), np.rint(nll * float(2 ** 36)).astype(np.int64),
                np.rint((m - yd) ** 2 * float(2 ** 40)).astype(np.int64), (lab == yy).astype(np.int64),
                (lab & yy).astype(np.int64), lab.astype(np.int64)]
        for f in range(int(n_folds)):
            out[f, q] = [int(v[fo == f].sum()) for v in cols]
    return out


def golden_select(predictions, y, loss: str = "nll", k_max: Optional[int] = None, replacement: bool = False):
    """Literal greedy forward selection on :func:`golden_mix`: ``(order, counts_path, train_loss)``."""
    p = M.as_2d(np.asarray(predictions))
    t_count = p.shape[0]
    k_max = t_count if k_max is None else int(k_max)
    col = 2 if loss == "nll" else 3
    scale = float(2 ** 36) if loss == "nll" else float(2 ** 40)
    cur = np.zeros(t_count, np.int64)
    order, path, losses = [], [], []
    for _ in range(k_max):
        best, best_m, best_n = None, -1, 1
        for m in range(t_count):
            if cur[m] and not replacement:
                continue
            row = golden_mix(p, y, (cur + np.eye(t_count, dtype=np.int64)[m])[None])[0, 0]
            if best is None or row[col] < best:
                best, best_m, best_n = int(row[col]), m, int(row[0])
        cur = cur.copy()
        cur[best_m] += 1
        order.append(best_m)
        path.append(cur)
        losses.append(best / scale / best_n if best_n else np.nan)
    return np.array(order, np.int64), np.stack(path), np.array(losses)


# ===================== Sums: kernel or emulation, one all-reduce under a process group =====================
class PairSums(NamedTuple):
    """The integer pair table of a prediction set: ``table`` (T, T, 3) int64 and the valid / positive windows."""
    table: np.ndarray
    n_valid: int
    n_y1: int


class _Sums:
    """The two reductions over one prediction set.  CUDA predictions go through the HIP kernels, anything else
    through the emulation; under an active process group every rank reduces its contiguous window shard and
    the integer arrays travel in one all-reduce per call."""

    def __init__(self, predictions, y, fold=None, n_folds: int = 1, distributed: Optional[bool] = None):
        torch = _torch()
        from . import distributed as DD

        MB = _ops()
        p2 = C._as_tensor_2d(predictions).contiguous()
        yy = torch.as_tensor(C._labels(y))
        t_count, n = p2.shape
        if len(yy) != n:
            raise ValueError(f"Mismatch between prediction samples ({n}) and label samples ({len(yy)})")
        if t_count > MB.MAX_T:
            raise ValueError(f"at most {MB.MAX_T} members, got {t_count}")
        if not 1 <= int(n_folds) <= MB.MAX_F:
            raise ValueError(f"n_folds must be in 1..{MB.MAX_F}")
        fd = None
        if fold is not None:
            codes = np.asarray(fold).reshape(-1)
            if len(codes) != n:
                raise ValueError(f"fold must have one code per window ({n})")
            if codes.size and (codes.min() < 0 or codes.max() >= int(n_folds)):
                raise ValueError(f"fold codes must lie in 0..{int(n_folds) - 1}")
            fd = torch.as_tensor(codes.astype(np.uint8))
        self.dist_on = DD.active() if distributed is None else bool(distributed)
        if self.dist_on:
            import torch.distributed as dist

            from ..parallel import dist as pdist

            s, e = pdist.shard_range(n, dist.get_rank(), dist.get_world_size())
            p2, yy, fd = p2[:, s:e].contiguous(), yy[s:e], None if fd is None else fd[s:e]
        dev = p2.device
        self.p, self.y, self.fold = p2, yy.to(dev), None if fd is None else fd.to(dev)
        self.t_count, self.n_folds = t_count, int(n_folds)

    def _reduce(self, arrays, name: str):
        if not self.dist_on:
            return [a.cpu().numpy() for a in arrays]
        torch = _torch()
        import torch.distributed as dist

        from ..parallel import comm
        from . import distributed as DD

        flat = torch.cat([a.reshape(-1) for a in arrays]).to(DD._comm_device())
        comm.run(name, flat, lambda: dist.all_reduce(flat))
        out, lo = [], 0
        for a in arrays:
            out.append(flat[lo:lo + a.numel()].reshape(a.shape).cpu().numpy())
            lo += a.numel()
        return out

    def pairs(self) -> PairSums:
        torch = _torch()
        MB = _ops()
        if self.p.shape[1]:
            table, head = (MB.pairs if self.p.is_cuda else MB.pairs_eager)(self.p, self.y)
        else:
            table = torch.zeros(self.t_count, self.t_count, 3, dtype=torch.int64)
            head = torch.zeros(2, dtype=torch.int64)
        table, head = self._reduce([table, head], "members_pairs_all_reduce")
        return PairSums(table, int(head[0]), int(head[1]))

    def mix(self, counts: np.ndarray) -> np.ndarray:
        """(Q, T) integer counts -> (F, Q, 7) int64; equal rows are reduced once."""
        torch = _torch()
        MB = _ops()
        counts = np.asarray(counts, np.int64).reshape(-1, self.t_count)
        uniq, inverse = np.unique(counts, axis=0, return_inverse=True)
        if self.p.shape[1]:
            out = (MB.mix if self.p.is_cuda else MB.mix_eager)(self.p, self.y, torch.as_tensor(uniq), self.fold,
                                                               self.n_folds)
        else:
            out = torch.zeros(self.n_folds, len(uniq), MB.N_MIX_COLS, dtype=torch.int64)
        return self._reduce([out], "members_mix_all_reduce")[0][:, np.asarray(inverse).reshape(-1)]


def on_device(predictions):
    """The predictions as a (T, N) tensor, on the GPU when there is one (the CLI loads NumPy dumps)."""
    p2 = C._as_tensor_2d(predictions)
    return p2.to("cuda") if C._gpu_ok() and not p2.is_cuda else p2


# ===================== Public API =====================
def member_pairs(predictions, y) -> PairSums:
    """The integer pair table of a prediction set, the input of :func:`subset_brier`."""
    return _Sums(predictions, y).pairs()


def member_table(predictions, y) -> Dict[str, np.ndarray]:
    """Per member (arrays of length T): ``accuracy``, ``sensitivity``, ``specificity``, ``nll``, ``brier`` of the
    member alone, and ``loo_nll_delta`` / ``loo_brier_delta``, the loss of the ensemble without the member minus
    the loss with all T (positive: the ensemble is worse off without it; NaN at T = 1).  Also the scalars
    ``ensemble_nll``, ``ensemble_brier``, ``ensemble_accuracy`` and ``n_valid``.  One reduction with the T unit
    rows, the T leave-one-out rows and the all-ones row."""
    s = _Sums(predictions, y)
    t_count = s.t_count
    eye = np.eye(t_count, dtype=np.int64)
    rows = [eye, np.ones((1, t_count), np.int64)] + ([1 - eye] if t_count > 1 else [])
    f = _ops().finalize_mix(s.mix(np.concatenate(rows))[0])
    out = {k: f[k][:t_count] for k in ("accuracy", "sensitivity", "specificity", "nll", "brier")}
    for k in LOSSES:
        out[f"ensemble_{k}"] = float(f[k][t_count])
        out[f"loo_{k}_delta"] = f[k][t_count + 1:] - f[k][t_count] if t_count > 1 else np.full(1, np.nan)
    out["ensemble_accuracy"] = float(f["accuracy"][t_count])
    out["n_valid"] = int(f["n_valid"][t_count])
    return out


def _pair_mean(m: np.ndarray) -> float:
    """Mean over the pairs a < b; NaN without pairs or when a pair's value is NaN."""
    iu = np.triu_indices(m.shape[0], 1)
    return float(np.mean(m[iu])) if len(iu[0]) else float("nan")


def _diversity(ps: PairSums) -> Dict:
    out = _ops().finalize_pairs(ps.table, np.array([ps.n_valid, ps.n_y1]))
    t_count = ps.table.shape[0]
    for k in MEANS:
        out[f"mean_{k}"] = _pair_mean(out[k])
    out["kw_variance"] = (t_count - 1) / (2.0 * t_count) * out["mean_disagreement"]
    n = float(ps.n_valid)
    g = ps.table[..., 2].astype(np.float64)
    scale = float(_ops().BRIER_SCALE)
    out["ensemble_brier"] = float(g.sum() / (t_count * t_count * n * scale)) if n else float("nan")
    out["member_brier"] = np.diagonal(g) / (n * scale) if n else np.full(t_count, np.nan)
    out["mean_member_brier"] = float(np.mean(out["member_brier"]))
    out["ambiguity"] = out["mean_member_brier"] - out["ensemble_brier"]
    return out


def member_diversity(predictions, y) -> Dict:
    """Pairwise (T, T) float64 matrices ``disagreement``, ``double_fault``, ``q_statistic``,
    ``error_correlation``, ``kappa`` (each also ``_y0`` / ``_y1``: restricted to one class) and
    ``residual_correlation``; their means over the pairs a < b as ``mean_*`` (NaN at T = 1);
    ``kw_variance = (T - 1) / (2 T) x mean_disagreement`` (Kohavi-Wolpert); and the Krogh-Vedelsby decomposition
    of the squared loss from the residual Gram G: ``ensemble_brier = 1' G 1 / (T^2 n)``, ``mean_member_brier``
    and ``ambiguity = mean_member_brier - ensemble_brier``, the mean squared distance of the members from the
    ensemble mean."""
    return _diversity(_Sums(predictions, y).pairs())


def subset_brier(pairs: PairSums, counts) -> np.ndarray:
    """The Brier score of the integer-weighted sub-ensembles ``counts`` ((T,) or (Q, T)) from the residual Gram
    alone, ``c' G c / (k^2 n)``: no pass over the data.  It differs from the ``brier_q`` column of the mixture
    sums by the quantisation only, at most half a quantum of 2^-40 per window on either side."""
    c = np.asarray(counts, np.float64)
    g = pairs.table[..., 2].astype(np.float64)
    k = c.sum(-1)
    val = np.einsum("...a,ab,...b->...", c, g, c)
    den = k * k * float(pairs.n_valid) * float(_ops().BRIER_SCALE)
    return np.where(den > 0, val / np.where(den > 0, den, 1.0), np.nan)


@dataclasses.dataclass
class MemberSelection:
    """A greedy selection path.  ``order[j]`` is the member added at step j, ``counts_path[j]`` the (T,) integer
    counts after it and ``train_loss[j]`` the mean loss of that sub-ensemble over the windows it was selected
    on: all valid windows.  When cross-fitted, ``fold_orders[f]`` is the path selected without fold f,
    ``heldout_loss_folds[f, j]`` its mean loss on fold f and ``heldout_loss[j]`` the mean over all windows, each
    scored by the path that did not see it."""
    loss: str
    replacement: bool
    n_members: int
    order: np.ndarray
    counts_path: np.ndarray
    train_loss: np.ndarray
    n_folds: int = 1
    seed: int = 2025
    heldout_loss: Optional[np.ndarray] = None
    heldout_loss_folds: Optional[np.ndarray] = None
    fold_orders: Optional[np.ndarray] = None

    def _k(self, k: int) -> int:
        if not 1 <= int(k) <= len(self.order):
            raise ValueError(f"k must be in 1..{len(self.order)}")
        return int(k)

    def subset(self, k: int) -> List[int]:
        """The distinct members among the first k picks, ascending (what ``load_ensemble`` needs)."""
        return sorted(set(int(m) for m in self.order[:self._k(k)]))

    def apply(self, predictions, k: int):
        """The ``(k, N, 1)`` prediction set of the first k picks, of the input's kind; a member picked twice
        (``replacement=True``) is there twice, so the set's mean is the mixture ``counts_path[k - 1]``."""
        torch = _torch()
        idx = np.asarray(self.order[:self._k(k)], np.int64)
        if isinstance(predictions, torch.Tensor):
            p = predictions if predictions.dim() == 3 else C._as_tensor_2d(predictions)[..., None]
            rows = p.shape[0]
        else:
            p = np.asarray(predictions)
            p = p if p.ndim == 3 else M.as_2d(p)[..., None]
            rows = p.shape[0]
        if rows != self.n_members:
            raise ValueError(f"the selection was made on {self.n_members} members, the set has {rows}")
        return p[torch.as_tensor(idx, device=p.device)] if isinstance(p, torch.Tensor) else p[idx]

    def save(self, path: str) -> str:
        """``.npz``: the arrays and one JSON string; nothing is pickled."""
        if not path.endswith(".npz"):
            path += ".npz"
        meta = {"format": 1, "loss": self.loss, "replacement": bool(self.replacement), "n_members": int(self.n_members),
                "n_folds": int(self.n_folds), "seed": int(self.seed)}
        arrays = {k: np.asarray(getattr(self, k)) for k in ("order", "counts_path", "train_loss", "heldout_loss",
                                                            "heldout_loss_folds", "fold_orders")
                  if getattr(self, k) is not None}
        np.savez(path, meta=np.array(json.dumps(meta)), **arrays)
        return path

    @classmethod
    def load(cls, path: str) -> "MemberSelection":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"][()]))
            arrays = {k: np.array(z[k]) for k in z.files if k != "meta"}
        meta.pop("format", None)
        return cls(**meta, **arrays)


def _greedy(sums: _Sums, loss: str, k_max: int, replacement: bool):
    """All paths of a selection together: path 0 is selected on every fold; with F > 1 folds, path 1 + f on the
    folds other than f.  One reduction per step over the candidate rows of every path (the sums are kept per
    fold, so the paths share it)."""
    MB = _ops()
    t_count, n_f = sums.t_count, sums.n_folds
    col = MB.MIX[loss + "_q"]
    scale = float(MB.NLL_SCALE if loss == "nll" else MB.BRIER_SCALE)
    n_paths = 1 + (n_f if n_f > 1 else 0)
    cur = np.zeros((n_paths, t_count), np.int64)
    order = np.zeros((n_paths, k_max), np.int64)
    paths = np.zeros((n_paths, k_max, t_count), np.int64)
    train = np.full((n_paths, k_max), np.nan)
    held = np.full((n_paths, k_max), np.nan)
    held_q = np.zeros((n_paths, k_max, 2), np.int64)
    eye = np.eye(t_count, dtype=np.int64)
    for j in range(k_max):
        cand = [[m for m in range(t_count) if replacement or cur[p, m] == 0] for p in range(n_paths)]
        rows = np.concatenate([cur[p][None] + eye[cand[p]] for p in range(n_paths)])
        out = sums.mix(rows)   # (F, rows, 7)
        lo = 0
        for p in range(n_paths):
            part = out[:, lo:lo + len(cand[p])]
            lo += len(cand[p])
            keep = np.ones(n_f, bool)
            if p > 0:
                keep[p - 1] = False
            loss_q, n_q = part[keep][..., col].sum(0), part[keep][..., 0].sum(0)
            best = int(np.argmin(loss_q))   # integers; the first minimum is the lowest member index
            m = cand[p][best]
            cur[p, m] += 1
            order[p, j] = m
            train[p, j] = loss_q[best] / scale / n_q[best] if n_q[best] else np.nan
            if p > 0:
                hq, hn = int(part[p - 1, best, col]), int(part[p - 1, best, 0])
                held_q[p, j] = hq, hn
                held[p, j] = hq / scale / hn if hn else np.nan
        paths[:, j] = cur
    pooled = None
    if n_f > 1:
        tot = held_q[1:].sum(0)
        pooled = np.where(tot[:, 1] > 0, tot[:, 0] / scale / np.maximum(tot[:, 1], 1), np.nan)
    return order, paths, train, held, pooled


def select_members(predictions, y, loss: str = "nll", k_max: Optional[int] = None, replacement: bool = False,
                   groups=None, n_folds: int = 1, seed: int = 2025, fold=None) -> MemberSelection:
    """Greedy forward selection of ensemble members (Caruana et al. 2004).

    Step j scores "current counts + one of member m" for every admissible m in one reduction and adds the
    member with the smallest integer loss sum over the selection windows (``loss``: ``"nll"`` or ``"brier"``);
    ties go to the lowest member index.  Without ``replacement`` a member is picked once and ``k_max`` is at
    most T; with it members may repeat (at most 255 times).  With ``n_folds > 1`` the windows are folded by
    ``assign_folds(groups, n_folds, seed)`` (a patient is never split; ``fold`` overrides it with given codes):
    fold f's path is selected on the other folds and scored on fold f, all in the same launches."""
    from .recalibration import assign_folds

    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}")
    t_count, n = C._as_tensor_2d(predictions).shape
    k_max = t_count if k_max is None else int(k_max)
    if k_max < 1 or (not replacement and k_max > t_count) or k_max > _ops().MAX_COUNT:
        raise ValueError("k_max must be in 1..T without replacement, in 1..255 with it")
    n_f = int(n_folds)
    codes = None
    if n_f > 1:
        codes = assign_folds(groups, n_f, seed, n) if fold is None else np.asarray(fold).reshape(-1)
    sums = _Sums(predictions, y, codes, n_f if n_f > 1 else 1)
    order, paths, train, held, pooled = _greedy(sums, loss, k_max, bool(replacement))
    sel = MemberSelection(loss=loss, replacement=bool(replacement), n_members=t_count, order=order[0],
                          counts_path=paths[0], train_loss=train[0], n_folds=n_f if n_f > 1 else 1, seed=int(seed))
    if n_f > 1:
        sel.heldout_loss, sel.heldout_loss_folds, sel.fold_orders = pooled, held[1:], order[1:]
    return sel


def _needed(loss_path: np.ndarray, target: float, tolerance: float) -> int:
    """Smallest k from which on ``loss_path[k - 1] <= target + tolerance``; the last k always qualifies."""
    ok = loss_path <= target + tolerance
    ok[-1] = True
    bad = np.flatnonzero(~ok)
    return int(bad[-1] + 2) if bad.size else 1


def evaluate_members(predictions, y, evaluation_label: str = "Members", patient_ids=None, n_folds: int = 5,
                     n_orders: int = 100, counts: Optional[Sequence[int]] = None,
                     tolerance: float = DEFAULT_TOLERANCE, random_state: Optional[int] = 2025,
                     output_dir: Optional[str] = "./uq_plots/members", make_plots: bool = True,
                     return_details: bool = False):
    """Diversity, member ranking and pruning curves of one prediction set, as one flat dictionary.

    The diversity means of :func:`member_diversity`, ``kw_variance``, ``ensemble_nll`` / ``ensemble_brier``,
    ``mean_member_nll`` / ``mean_member_brier``, ``ambiguity``, ``best_member`` / ``worst_member`` (by the
    member's own NLL).  For each loss and every count k of ``default_counts(T, counts)``:
    ``greedy_{loss}_at_{k}``, the loss of the k greedily chosen members (held out, pooled over the folds, when
    ``n_folds > 1``: every window is scored by the path selected without its patient's fold; with
    ``n_folds <= 1`` the loss on the selection windows themselves), ``first_{loss}_at_{k}``, the first k members
    as given, and ``random_{loss}_at_{k}_mean`` / ``_ci_lower`` / ``_ci_upper``, the mean and the 2.5 / 97.5
    percentiles over the random k-subsets of ``subset_orders(T, n_orders, random_state)``.
    ``members_needed_{loss}`` is the smallest k such that at every k' >= k in 1..T the greedy loss is at most
    the all-T loss plus ``tolerance``: an absolute margin in the loss's own unit, 0.001 by default (nats per
    window for the NLL, squared probability for the Brier score).

    With ``output_dir``: ``member_table_{label}.csv``, ``member_curve_{label}.csv`` and, unless ``make_plots`` is
    off, a heat map of the pairwise disagreement and the pruning curves.  ``return_details=True`` returns
    ``(dict, details)`` with the member table and the two ``MemberSelection`` objects (``details["table"]``,
    ``details["selection"][loss]``), so that a caller needs no second pass over the data."""
    MB = _ops()
    base = _Sums(predictions, y)
    t_count = base.t_count
    seed = 2025 if random_state is None else int(random_state)
    div = _diversity(base.pairs())
    table = member_table(predictions, y)
    final: Dict[str, float] = {f"mean_{k}": div[f"mean_{k}"] for k in MEANS}
    final.update(kw_variance=div["kw_variance"], ensemble_nll=table["ensemble_nll"],
                 ensemble_brier=table["ensemble_brier"], mean_member_nll=float(np.mean(table["nll"])),
                 mean_member_brier=float(np.mean(table["brier"])), ambiguity=div["ambiguity"],
                 best_member=int(np.argmin(table["nll"])), worst_member=int(np.argmax(table["nll"])))
    cs = default_counts(t_count, counts)
    orders = subset_orders(t_count, n_orders, random_state)
    rows = []
    for order in orders:
        for k in cs:
            c = np.zeros(t_count, np.int64)
            c[order[:k]] = 1
            rows.append(c)
    fm = MB.finalize_mix(base.mix(np.stack(rows))[0])
    curve = [{"N": int(k)} for k in cs]
    bands, selections = {}, {}
    cross = int(n_folds) > 1 and t_count > 1
    for loss in LOSSES:
        v = fm[loss].reshape(len(orders), len(cs))
        rnd = v[1:] if len(orders) > 1 else v
        # a mean of equal values may round one ulp away from them (every k = T subset is the whole ensemble): keep it
        # inside the values' range, as evaluate_convergence does
        mean = np.clip(rnd.mean(0), rnd.min(0), rnd.max(0))
        lo, hi = np.percentile(rnd, 2.5, axis=0), np.percentile(rnd, 97.5, axis=0)
        sel = selections[loss] = select_members(predictions, y, loss=loss, groups=patient_ids, n_folds=int(n_folds) if cross else 1,
                             seed=seed)
        greedy = sel.heldout_loss if cross else sel.train_loss
        bands[loss] = (greedy[cs - 1], v[0], mean, lo, hi)
        for j, k in enumerate(cs):
            final[f"greedy_{loss}_at_{k}"] = float(greedy[k - 1])
            final[f"first_{loss}_at_{k}"] = float(v[0, j])
            final[f"random_{loss}_at_{k}_mean"], final[f"random_{loss}_at_{k}_ci_lower"] = float(mean[j]), float(lo[j])
            final[f"random_{loss}_at_{k}_ci_upper"] = float(hi[j])
            curve[j].update({f"greedy_{loss}": float(greedy[k - 1]), f"first_{loss}": float(v[0, j]),
                             f"random_{loss}_mean": float(mean[j]), f"random_{loss}_lower": float(lo[j]),
                             f"random_{loss}_upper": float(hi[j])})
        final[f"members_needed_{loss}"] = _needed(np.array(greedy, np.float64), final[f"ensemble_{loss}"], tolerance)
        final[f"greedy_order_{loss}"] = ",".join(str(int(m)) for m in sel.order)
    if output_dir:
        os.makedirs(output_dir, exist_ok=True)
        cols = ("accuracy", "sensitivity", "specificity", "nll", "brier", "loo_nll_delta", "loo_brier_delta")
        frame = pd.DataFrame({"member": np.arange(t_count), **{k: np.resize(table[k], t_count) for k in cols}})
        frame.to_csv(os.path.join(output_dir, f"member_table_{evaluation_label}.csv"), index=False)
        pd.DataFrame(curve).to_csv(os.path.join(output_dir, f"member_curve_{evaluation_label}.csv"), index=False)
        if make_plots:
            plot_pairwise(div["disagreement"], evaluation_label, output_dir)
            plot_pruning(cs, bands, evaluation_label, output_dir, cross)
    return (final, {"table": table, "selection": selections}) if return_details else final


# ===================== Plots =====================
def plot_pairwise(matrix: np.ndarray, label: str, output_dir: str, name: str = "disagreement"):
    """Heat map of a pairwise (T, T) statistic."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig = plt.figure(figsize=(6, 5))
    plt.imshow(matrix, cmap="viridis")
    plt.colorbar(label=name)
    plt.xlabel("member")
    plt.ylabel("member")
    plt.title(f"Pairwise {name} - {label}")
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"member_pairwise_{label}.png"), bbox_inches="tight")
    plt.close(fig)


def plot_pruning(counts, bands: Dict, label: str, output_dir: str, heldout: bool):
    """Loss against the number of members: greedy, the first k as given, and the band of random k-subsets."""
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    fig, axes = plt.subplots(1, len(bands), figsize=(6 * len(bands), 4.5))
    for ax, (loss, (greedy, first, mean, lo, hi)) in zip(np.atleast_1d(axes), bands.items()):
        ax.fill_between(counts, lo, hi, alpha=0.25, label="95% of random subsets")
        ax.plot(counts, mean, "-", label="mean over random subsets")
        ax.plot(counts, first, "o--", ms=3, label="first k as given")
        ax.plot(counts, greedy, "s-", ms=3, label="greedy" + (" (held out)" if heldout else " (selection windows)"))
        ax.set_xlabel("Members used")
        ax.set_ylabel(loss)
        ax.grid(True, alpha=0.3)
        ax.legend(fontsize=8)
    fig.suptitle(f"Ensemble pruning - {label}")
    fig.tight_layout()
    fig.savefig(os.path.join(output_dir, f"member_pruning_{label}.png"), bbox_inches="tight")
    plt.close(fig)
