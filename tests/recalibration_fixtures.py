"""Shared inputs of the recalibration tests: an over-confident synthetic ensemble and its edge-case variants.

The true logit is N(-1, 1.5), the label Bernoulli of its sigmoid, a member's logit ``2.5 z + 0.4 + noise``: the
members are over-confident and shifted, so every method has something to correct.  Everything the tests assume of
the fixtures is asserted here of the float64 golden alone (:func:`golden_facts`), so a test cannot hide a failure
behind its own slack.
"""
from __future__ import annotations

import functools

import numpy as np

from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import recalibration as RC

KINDS = ("plain", "clip", "nan", "label2")


def ensemble(n: int, T: int, seed: int = 0, noise: float = 0.7):
    """``(probs (T, n) float32, y (n,) int64)``."""
    rng = np.random.default_rng(seed)
    z = rng.normal(-1.0, 1.5, n)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.int64)
    logit = 2.5 * z[None] + 0.4 + noise * rng.standard_normal((T, n))
    return (1.0 / (1.0 + np.exp(-logit))).astype(np.float32), y


def variant(n: int, T: int, kind: str = "plain", seed: int = 0):
    """The ensemble with an edge case planted: ``clip`` p exactly 0 and 1, ``nan`` one NaN window (and an inf),
    ``label2`` one label of 2."""
    p, y = ensemble(n, T, seed)
    if kind == "clip":
        p[0, 0] = 0.0
        p[T - 1, n - 1] = 1.0
        if n > 2:
            p[:, n // 2] = 1.0
    elif kind == "nan":
        p[T // 2, n // 3] = np.nan
        if n > 4:
            p[0, n - 2] = np.inf
    elif kind == "label2":
        y[n // 2] = 2
    elif kind != "plain":
        raise ValueError(kind)
    return p, y


def patients(n: int, n_patients: int, seed: int = 1) -> np.ndarray:
    """Patient ids, contiguous per patient (as the detail CSVs have them), of unequal sizes."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n), size=n_patients - 1, replace=False))
    return np.searchsorted(cuts, np.arange(n), side="right").astype(np.int64) + 100


def fold_codes(n: int, F: int, layout: str = "grouped", seed: int = 2) -> np.ndarray:
    """int32 codes in [0, F): ``grouped`` by contiguous patients, ``shuffled`` per window; from 8 windows on, one
    code of -1 and one of F (both to be skipped)."""
    if F == 1:
        codes = np.zeros(n, np.int32)
    elif layout == "grouped":
        P = max(min(n // 3, 40), 1)
        pid = patients(n, P, seed) if P > 1 else np.zeros(n, np.int64)
        codes = ((pid * 7 + 3) % F).astype(np.int32)
    else:
        codes = np.random.default_rng(seed).integers(0, F, n).astype(np.int32)
    if n >= 8:
        codes[1], codes[n - 3] = -1, F
    return codes


def candidates(Q: int, seed: int = 3) -> np.ndarray:
    """(Q, 3) float64: the identity first, then points around it (a, b in [0.2, 1.6], c in [-1, 1])."""
    rng = np.random.default_rng(seed)
    th = np.stack([rng.uniform(0.2, 1.6, Q), rng.uniform(0.2, 1.6, Q), rng.uniform(-1.0, 1.0, Q)], axis=1)
    th[0] = (1.0, 1.0, 0.0)
    return th


FIT_N, FIT_T, FIT_PATIENTS, FIT_FOLDS = 1200, 7, 30, 5


@functools.lru_cache(maxsize=None)
def fit_set():
    p, y = ensemble(FIT_N, FIT_T, seed=11)
    return p, y, patients(FIT_N, FIT_PATIENTS)


@functools.lru_cache(maxsize=None)
def golden_facts(method: str, objective: str):
    """The golden fit of :func:`fit_set`, with the facts the tests lean on asserted of the golden itself."""
    p, y, _ = fit_set()
    g = RC.golden_fit(p, y, method, objective)
    eig = np.linalg.eigvalsh(g["H"])
    assert eig[0] > 0, "the golden Hessian at the golden optimum must be positive definite"
    assert eig[-1] / eig[0] < 1e3, f"condition number {eig[-1] / eig[0]:.3g}"
    assert g["theta"][0] >= 0 and g["theta"][1] >= 0, "no a or b may be negative on the fixture"
    assert np.linalg.norm(g["g"]) / g["n_valid"] < 1e-9, "the golden must sit at a stationary point"
    return g


@functools.lru_cache(maxsize=None)
def fold_facts():
    """The fold codes of the fit set's patients; both classes present in every training complement."""
    p, y, pid = fit_set()
    codes = RC.assign_folds(pid, FIT_FOLDS, 2025)
    for f in range(FIT_FOLDS):
        yc = y[codes != f]
        assert 0 < yc.sum() < len(yc), f"fold {f}: the complement lacks a class"
    return codes


def theta_bound(g) -> float:
    """``2 x 1e-8 x n_valid / lambda_min(H_golden)``: the stop criterion through the golden's own Hessian."""
    return 2.0 * 1e-8 * g["n_valid"] / float(np.linalg.eigvalsh(g["H"])[0])
