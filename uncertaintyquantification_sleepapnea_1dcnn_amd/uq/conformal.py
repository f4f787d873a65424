"""Split conformal prediction sets for the apnea classifier, and their coverage over patient splits.

Calibration and recalibration describe uncertainty; a conformal set carries a guarantee: it contains the true
label of a new window with probability at least ``1 - alpha`` whenever calibration and new windows are
exchangeable, whatever the model.  With two labels a set is empty, ``{normal}``, ``{apnea}`` or both; the empty
and the two-label sets are the windows to refer to a human scorer.

Definitions (``golden_conformal_split`` implements them literally)
------------------------------------------------------------------
``p`` is the fp32 mean over the T passes or members of a prediction set (the MEAN row of ``uq_reduce``) and
``y`` in {0, 1}.  Windows with a non-finite ``p`` are dropped from calibration and from every count (the number
kept is reported as ``n_valid``); ``predict_sets`` gives them the full set.

Miscoverage levels are integers, ``alpha_ppm = round(alpha 10^6)`` in 1..999,999, and the conformal rank is

    ``k(n) = ((n + 1)(10^6 - alpha_ppm) + 10^6 - 1) // 10^6``        (int64)

so that exact products (n = 19, alpha = 0.05: k = 19) do not hang on how a floating ``(n + 1)(1 - alpha)`` happens
to round before its ``ceil``.  ``k > n`` means an infinite threshold: the label is always in the set.

``mode="class_conditional"`` (Mondrian, the default) works in probability space, without ``1 - p``:
``tau0`` is the k(n_cal,0)-th smallest ``p`` of the calibration windows with y = 0 and ``tau1`` the k(n_cal,1)-th
LARGEST ``p`` of those with y = 1; label 0 is in the set iff ``p <= tau0``, label 1 iff ``p >= tau1`` (ties are in:
deterministic and conservative).  Each class is covered separately, which matters on an unbalanced test set.
(Stated through ``1 - p64 <= q`` instead, distinct probabilities below 2^-29 would collapse into one tie group.)

``mode="marginal"`` works on float64 scores ``s(x, 0) = p64``, ``s(x, 1) = 1.0 - p64``: ``qhat`` is the k(n_cal)-th
smallest true-label score of all calibration windows and label c is in the set iff ``s(x, c) <= qhat``.

Set code: bit c is set iff label c is in the set: 0 empty, 1 ``{normal}``, 2 ``{apnea}``, 3 both.

Evaluation over splits
----------------------
``evaluate_conformal`` answers "what coverage and set sizes would other calibration / test splits of my patients
have given?".  A split does not change the order of ``p``: the windows are sorted once and, with ``e0`` the number
of sorted windows with label 0 in the set, ``s1`` the number with label 1 not in it and ``T_z(c)`` the test windows
of class z among sorted positions [0, c), per class z

    ``n_test_z = T_z(n)``, ``incl0_z = T_z(e0)``, ``incl1_z = n_test_z - T_z(s1)``,
    ``both_z = T_z(e0) - T_z(s1)`` if ``e0 >= s1`` else 0,  ``empty_z = T_z(s1) - T_z(e0)`` if ``s1 > e0`` else 0.

Class-conditional: ``e0`` is the end of the tie group of the selected class-0 calibration window (n if the
threshold is infinite), ``s1`` the start of the tie group of the selected class-1 window (0).  Marginal: ``qhat``
comes from a second sort, of the true-label scores, ``e0 = searchsorted(p64, qhat, right)`` and
``s1 = n - searchsorted((1.0 - p64)[::-1], qhat, right)``.  The rank selections and the prefix counts of all splits
and levels run on the device (``ops/conformal.py`` / ``csrc/uq_conformal.hip``).

Roles are a pure function of coordinates (as the dropout masks and bootstrap draws are).  A *unit* is a patient
when ``patient_ids`` is given, else a window; unit u calibrates in split r iff
``split_hash(seed, r, u) < floor(cal_fraction 2^32)`` (``ops/rng.py``), every other unit is a test unit.
``cluster="pooled"`` (default): all windows of a calibration unit calibrate.  The guarantee is then approximate,
because the windows of a patient are dependent.  ``cluster="subsample"``: one window per calibration patient
calibrates, the one whose index among the patient's valid windows equals ``(split_hash2(seed, r, u) count_u) >> 32``;
the patient's other windows are neither calibration nor test.  This variant has the exact finite-sample guarantee
under patient exchangeability.

Class-conditional sets are invariant under any strictly increasing map of ``p``, so temperature / Platt
recalibration (monotone maps) does not change them; marginal sets are not invariant.

Multi-rank: thresholds are order statistics and not shard-additive; as in ``discrimination.py`` compute from the
gathered per-window means.
"""
from __future__ import annotations

import dataclasses
import json
import os
import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import calibration as C

MODES = ("class_conditional", "marginal")
CLUSTERS = ("pooled", "subsample")
DEFAULT_ALPHAS = (0.01, 0.025, 0.05, 0.1, 0.15, 0.2)
PPM = 10 ** 6


def _torch():
    import torch

    return torch


def _ops():
    from ..ops import conformal

    return conformal


def _check_mode(mode: str) -> None:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")


def _labels01(y) -> np.ndarray:
    torch = _torch()
    yy = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
    if yy.size and not np.all((yy == 0) | (yy == 1)):
        raise ValueError("labels must be 0 or 1")
    return yy.astype(np.int64)


# ===================== Golden: the literal per-window definition =====================
def golden_conformal_split(p, y, cal_mask, test_mask, alpha_ppm: int, mode: str = "class_conditional") -> Dict:
    """One split and one level straight from the definitions, window by window (NumPy).

    Returns the thresholds (``tau0``, ``tau1`` or ``qhat``), ``k`` and ``n_cal`` per stratum, ``sets`` (N,) uint8
    (the code of every window; 3 for a non-finite ``p``), ``counts`` (the ten integers of ``ops.conformal.COLS`` over
    the finite test windows) and the float64 metrics computed from the per-window sets."""
    _check_mode(mode)
    ops = _ops()
    p32 = np.asarray(p, np.float32).reshape(-1)
    yy = np.asarray(y).reshape(-1).astype(np.int64)
    fin = np.isfinite(p32)
    cal = np.asarray(cal_mask, bool).reshape(-1) & fin
    test = np.asarray(test_mask, bool).reshape(-1) & fin
    a = int(alpha_ppm)
    out: Dict = {}
    if mode == "class_conditional":
        c0 = np.sort(p32[cal & (yy == 0)])
        c1 = np.sort(p32[cal & (yy == 1)])[::-1]
        k0, k1 = int(ops.rank_k(len(c0), a)), int(ops.rank_k(len(c1), a))
        tau0 = float(c0[k0 - 1]) if k0 <= len(c0) else np.inf
        tau1 = float(c1[k1 - 1]) if k1 <= len(c1) else -np.inf
        with np.errstate(invalid="ignore"):
            in0, in1 = p32.astype(np.float64) <= tau0, p32.astype(np.float64) >= tau1
        out.update(tau0=tau0, tau1=tau1, k=(k0, k1), n_cal=(len(c0), len(c1)))
    else:
        p64 = p32.astype(np.float64)
        s0, s1 = p64, 1.0 - p64
        sc = np.sort(np.where(yy == 1, s1, s0)[cal])
        k = int(ops.rank_k(len(sc), a))
        qhat = float(sc[k - 1]) if k <= len(sc) else np.inf
        with np.errstate(invalid="ignore"):
            in0, in1 = s0 <= qhat, s1 <= qhat
        out.update(qhat=qhat, k=(k,), n_cal=(len(sc),))
    sets = (in0.astype(np.uint8) | (in1.astype(np.uint8) << 1))
    sets[~fin] = 3
    out["sets"] = sets
    counts = {}
    for z in (0, 1):
        m = test & (yy == z)
        counts[f"n_test_{z}"] = int(m.sum())
        counts[f"incl0_{z}"] = int((m & in0).sum())
        counts[f"incl1_{z}"] = int((m & in1).sum())
        counts[f"both_{z}"] = int((m & in0 & in1).sum())
        counts[f"empty_{z}"] = int((m & ~in0 & ~in1).sum())
    out["counts"] = counts
    st, yt = sets[test], yy[test]
    n = len(st)
    covered = ((st >> yt) & 1).astype(bool)
    size = (st & 1) + (st >> 1)
    single = size == 1

    def mean(v):
        return float(np.mean(v)) if len(v) else float("nan")

    out.update(coverage=mean(covered), coverage_class_0=mean(covered[yt == 0]), coverage_class_1=mean(covered[yt == 1]),
               share_empty=mean(size == 0), share_singleton=mean(single), share_both=mean(size == 2),
               mean_set_size=mean(size.astype(np.float64)), singleton_accuracy=mean(covered[single]), n_valid=n)
    return out


# ===================== Calibrate / predict =====================
@dataclasses.dataclass
class ConformalPredictor:
    """Fitted thresholds of one level.  ``tau0`` / ``tau1`` (class-conditional) or ``qhat`` (marginal) are float64
    and may be infinite; ``k`` and ``n_cal`` hold one entry per stratum (class 0, class 1; or the single one)."""
    mode: str
    alpha_ppm: int
    tau0: Optional[float]
    tau1: Optional[float]
    qhat: Optional[float]
    k: Tuple[int, ...]
    n_cal: Tuple[int, ...]

    @property
    def alpha(self) -> float:
        return self.alpha_ppm / PPM

    def predict_sets(self, preds):
        """(N,) uint8 set codes of a prediction set (NumPy, or a torch tensor on the input's device); a window
        with a non-finite mean gets the full set."""
        torch = _torch()
        p64 = _mean_probability(preds, "cuda" if C._use_device(preds) else None).double()
        if self.mode == "class_conditional":
            in0, in1 = p64 <= self.tau0, p64 >= self.tau1
        else:
            in0, in1 = p64 <= self.qhat, (1.0 - p64) <= self.qhat
        sets = in0.to(torch.uint8) | (in1.to(torch.uint8) << 1)
        sets = torch.where(torch.isfinite(p64), sets, torch.full_like(sets, 3))
        return sets.to(preds.device) if isinstance(preds, torch.Tensor) else sets.cpu().numpy()

    def scalars(self) -> Dict:
        return {"mode": self.mode, "alpha_ppm": int(self.alpha_ppm), "k": [int(v) for v in self.k],
                "n_cal": [int(v) for v in self.n_cal]}

    def save(self, path: str) -> str:
        """``.npz``: the float64 thresholds ``[tau0, tau1, qhat]`` (NaN = unused) and one JSON string; nothing is pickled."""
        if not path.endswith(".npz"):
            path += ".npz"
        thr = np.array([np.nan if v is None else v for v in (self.tau0, self.tau1, self.qhat)], np.float64)
        np.savez(path, thresholds=thr, meta=np.array(json.dumps(dict(self.scalars(), format=1))))
        return path

    @classmethod
    def load(cls, path: str) -> "ConformalPredictor":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"][()]))
            thr = np.array(z["thresholds"], np.float64)
        cc = meta["mode"] == "class_conditional"
        return cls(mode=meta["mode"], alpha_ppm=int(meta["alpha_ppm"]), tau0=float(thr[0]) if cc else None,
                   tau1=float(thr[1]) if cc else None, qhat=None if cc else float(thr[2]),
                   k=tuple(meta["k"]), n_cal=tuple(meta["n_cal"]))


def _mean_probability(preds, device=None):
    """(N,) fp32 torch tensor: the mean over T (``ops.uq.metrics`` MEAN row; the HIP kernel on the GPU)."""
    return C.per_window(preds, "pred_variance", device)[0]


def conformal_calibrate(preds, y, alpha: float = 0.1, mode: str = "class_conditional") -> ConformalPredictor:
    """Thresholds of level ``alpha`` from the calibration set ``(preds, y)``: order statistics of the mean
    probability (see the module docstring).  A class without calibration windows (class-conditional) or an empty
    set gives an infinite threshold and one warning."""
    torch = _torch()
    ops = _ops()
    _check_mode(mode)
    if np.ndim(alpha) != 0:
        raise ValueError("alpha must be one number")
    ppm = int(ops.alpha_to_ppm(alpha)[0])
    p = _mean_probability(preds, "cuda" if C._use_device(preds) else None)
    yy = torch.as_tensor(_labels01(y), device=p.device)
    if yy.numel() != p.numel():
        raise ValueError(f"Mismatch between prediction samples ({p.numel()}) and label samples ({yy.numel()})")
    fin = torch.isfinite(p)

    def kth(values, k):  # the k-th smallest, 1-based
        return float(torch.sort(values).values[k - 1])

    if mode == "class_conditional":
        c0, c1 = p[fin & (yy == 0)].double(), p[fin & (yy == 1)].double()
        n0, n1 = c0.numel(), c1.numel()
        k0, k1 = int(ops.rank_k(n0, ppm)), int(ops.rank_k(n1, ppm))
        if n0 == 0 or n1 == 0:
            warnings.warn("conformal_calibrate: a class has no calibration windows; its threshold is infinite "
                          "(the label is always in the set)", RuntimeWarning, stacklevel=2)
        tau0 = kth(c0, k0) if k0 <= n0 else float("inf")
        tau1 = kth(c1, n1 - k1 + 1) if k1 <= n1 else float("-inf")
        return ConformalPredictor(mode, ppm, tau0, tau1, None, (k0, k1), (n0, n1))
    p64 = p[fin].double()
    sc = torch.where(yy[fin] == 1, 1.0 - p64, p64)
    n = sc.numel()
    k = int(ops.rank_k(n, ppm))
    if n == 0:
        warnings.warn("conformal_calibrate: no calibration windows; the threshold is infinite", RuntimeWarning,
                      stacklevel=2)
    return ConformalPredictor(mode, ppm, None, None, kth(sc, k) if k <= n else float("inf"), (k,), (n,))


def conformal_metrics(sets, y, valid=None) -> Dict:
    """``coverage``, ``coverage_class_0/1``, ``share_empty``, ``share_singleton``, ``share_both``, ``mean_set_size``,
    ``singleton_accuracy`` and ``n_valid`` of set codes against the labels.  ``valid`` (N,) bool leaves windows out
    (those with a non-finite mean, to match :func:`evaluate_conformal`)."""
    torch = _torch()
    ops = _ops()
    s = np.asarray(sets.cpu() if isinstance(sets, torch.Tensor) else sets).reshape(-1).astype(np.int64)
    yy = _labels01(y)
    if len(s) != len(yy):
        raise ValueError(f"Mismatch between sets ({len(s)}) and label samples ({len(yy)})")
    if s.size and (s.min() < 0 or s.max() > 3):
        raise ValueError("set codes must be 0..3")
    keep = np.ones(len(s), bool) if valid is None else np.asarray(valid, bool).reshape(-1)
    in0, in1 = (s & 1) == 1, (s & 2) == 2
    counts = []
    for z in (0, 1):
        m = keep & (yy == z)
        counts += [m.sum(), (m & in0).sum(), (m & in1).sum(), (m & in0 & in1).sum(), (m & ~in0 & ~in1).sum()]
    fin = ops.finalize(np.array(counts, np.int64))
    return {k: (int(v) if k == "n_valid" else float(v)) for k, v in fin.items()}


# ===================== Evaluation over splits =====================
def unit_codes(n_total: int, patient_ids=None) -> Tuple[np.ndarray, int]:
    """((N,) int32 unit of every window, number of units): the index of its patient among the sorted unique ids,
    or the window's own index."""
    if patient_ids is None:
        return np.arange(n_total, dtype=np.int32), int(n_total)
    ids, inverse = np.unique(np.asarray(patient_ids).reshape(-1), return_inverse=True)
    if inverse.size != n_total:
        raise ValueError(f"Mismatch between prediction samples ({n_total}) and patient ids ({inverse.size})")
    return inverse.reshape(-1).astype(np.int32), len(ids)


def within_unit(codes: np.ndarray, valid: np.ndarray, n_units: int) -> Tuple[np.ndarray, np.ndarray]:
    """((N,) int32 index of every valid window among the valid windows of its unit, in window order (-1: not
    valid), (P,) int32 valid windows per unit)."""
    idx = np.nonzero(valid)[0]
    cv = codes[idx]
    order = np.argsort(cv, kind="stable")
    cs = cv[order]
    ucount = np.bincount(cv, minlength=n_units).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(ucount)[:-1]])
    within = np.full(len(codes), -1, np.int32)
    within[idx[order]] = (np.arange(len(cs)) - first[cs]).astype(np.int32)
    return within, ucount


def split_masks(p, seed: int, r: int, cal_fraction: float = 0.5, patient_ids=None,
                cluster: str = "pooled") -> Tuple[np.ndarray, np.ndarray]:
    """``(cal_mask, test_mask)`` (N,) bool of split ``r`` in window order: the roles :func:`evaluate_conformal`
    uses (windows with a non-finite ``p`` have neither role)."""
    torch = _torch()
    ops = _ops()
    if cluster not in CLUSTERS:
        raise ValueError(f"cluster must be one of {CLUSTERS}")
    pv = np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p, np.float32).reshape(-1)
    valid = np.isfinite(pv)
    codes, n_units = unit_codes(len(pv), patient_ids)
    within = ucount = None
    if cluster == "subsample" and patient_ids is not None:
        w, uc = within_unit(codes, valid, n_units)
        within, ucount = torch.as_tensor(w), torch.as_tensor(uc)
    cal, test = ops.roles_eager(seed, r, torch.as_tensor(codes), within, ucount, ops.cal_threshold(cal_fraction))
    return cal.numpy() & valid, test.numpy() & valid


def _prepare(p, y, patient_ids, cluster: str, mode: str) -> Dict:
    """Everything that does not depend on the split: the sort(s) and the role inputs in sorted order."""
    torch = _torch()
    from ..ops import rank

    dev = p.device
    yy = torch.as_tensor(_labels01(y), device=dev)
    pr = rank.prep(p, yy)
    perm, n = pr["perm"], pr["n_valid"]
    codes, n_units = unit_codes(p.numel(), patient_ids)
    unit = torch.as_tensor(codes, device=dev)[perm].contiguous()
    within = ucount = None
    if cluster == "subsample" and patient_ids is not None:
        valid = np.zeros(p.numel(), bool)
        valid[perm.cpu().numpy()] = True
        w, uc = within_unit(codes, valid, n_units)
        within, ucount = torch.as_tensor(w, device=dev)[perm].contiguous(), torch.as_tensor(uc, device=dev)
    out = {"n": n, "n_total": pr["n_total"], "unit": unit, "packed": pr["packed"], "within": within, "ucount": ucount}
    if mode == "class_conditional":
        out["group_start"], out["group_end"] = _ops().group_bounds((pr["packed"] & rank.START_BIT) != 0)
    else:
        p64 = pr["sorted"].double()
        score = torch.where((pr["packed"] & rank.Z_BIT) != 0, 1.0 - p64, p64)
        srt, order = torch.sort(score, stable=True)
        out.update(p64=p64.contiguous(), q64_rev=(1.0 - p64).flip(0).contiguous(), score=srt,
                   unit_s=unit[order].contiguous(), packed_s=pr["packed"][order].contiguous(),
                   within_s=None if within is None else within[order].contiguous())
    return out


def _split_counts(pp: Dict, seed: int, r0: int, n_splits: int, cal_thr: int, ppm, mode: str, segments: int = 0):
    """``(totals (R, 4) int32, counts (R, A, 10) int64)`` of splits ``r0 .. r0 + R - 1``: two device launches."""
    torch = _torch()
    ops = _ops()
    n, dev = pp["n"], pp["unit"].device
    n_alpha = ppm.numel()
    if n == 0 or n_splits == 0:
        return (torch.zeros(n_splits, 4, dtype=torch.int32, device=dev),
                torch.zeros(n_splits, n_alpha, 10, dtype=torch.int64, device=dev))
    if mode == "class_conditional":
        totals, member = ops.select(pp["unit"], pp["packed"], pp["within"], pp["ucount"], seed, r0, n_splits, cal_thr,
                                    ppm, 2, segments)
        m0, m1 = member[:, 0].long(), member[:, 1].long()
        e0 = torch.where(m0 >= 0, pp["group_end"][m0.clamp(min=0)], torch.full_like(m0, n))
        s1 = torch.where(m1 >= 0, pp["group_start"][m1.clamp(min=0)], torch.zeros_like(m1))
    else:
        totals, member = ops.select(pp["unit_s"], pp["packed_s"], pp["within_s"], pp["ucount"], seed, r0, n_splits,
                                    cal_thr, ppm, 1, segments)
        m = member[:, 0].long()
        inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
        qhat = torch.where(m >= 0, pp["score"][m.clamp(min=0)], inf)
        e0 = torch.searchsorted(pp["p64"], qhat, right=True)
        s1 = n - torch.searchsorted(pp["q64_rev"], qhat, right=True)
    cuts = torch.cat([e0, s1], dim=1).to(torch.int32)
    tz = ops.count(pp["unit"], pp["packed"], pp["within"], pp["ucount"], seed, r0, cal_thr, cuts, segments)
    return totals, ops.assemble(totals, tz, e0, s1)


def level_suffixes(alphas) -> list:
    """Key suffixes such as ``_at_0.10`` in the order given, with as many decimals (2, 3, 4 or 6) as write every
    level exactly and keep them distinct (the default levels: ``_at_0.010``, ``_at_0.025``, ...)."""
    a = np.asarray(alphas, np.float64).reshape(-1)
    for nd in (2, 3, 4, 6):
        out = [f"_at_{v:.{nd}f}" for v in a]
        if len(set(out)) == len(out) and all(abs(float(s[4:]) - v) < 5e-7 for s, v in zip(out, a)):
            break
    return out


def evaluate_conformal(preds, y, method_name: str = "Conformal", alphas: Sequence[float] = DEFAULT_ALPHAS,
                       n_splits: int = 1000, cal_fraction: float = 0.5, patient_ids=None, cluster: str = "pooled",
                       mode: str = "class_conditional", random_state: int = 2025, output_dir: Optional[str] = None,
                       make_plots: bool = True, return_details: bool = False):
    """Coverage and set sizes of split conformal prediction over ``n_splits`` random calibration / test splits.

    Returns a flat dictionary: for every metric m of ``ops.conformal.METRICS`` and level, ``{m}_at_{alpha}`` (the
    mean over the splits), ``..._ci_lower`` / ``..._ci_upper`` (their 2.5 / 97.5 percentiles) and
    ``coverage_violation_rate_at_{alpha}`` (the share of splits whose test coverage is below ``1 - alpha``, compared
    in integers), plus ``n_valid``, ``n_splits``, ``n_units`` and the mean calibration / test sizes.  Splits are by
    patient when ``patient_ids`` is given; without them a warning says that window splits ignore the correlation
    within a patient.  Two plots (coverage against ``1 - alpha`` with its band, set-type shares against alpha) go to
    ``output_dir`` (default ``./uq_plots``).  ``return_details``: also the per-split arrays ``totals`` (R, 4),
    ``counts`` (R, A, 10) and the (R, A) metrics."""
    torch = _torch()
    ops = _ops()
    _check_mode(mode)
    if cluster not in CLUSTERS:
        raise ValueError(f"cluster must be one of {CLUSTERS}")
    ppm_np = ops.alpha_to_ppm(alphas)
    if len(ppm_np) > ops.MAX_ALPHA:
        raise ValueError(f"at most {ops.MAX_ALPHA} miscoverage levels")
    if int(n_splits) < 1:
        raise ValueError("n_splits must be at least 1")
    cal_thr = ops.cal_threshold(cal_fraction)
    if patient_ids is None:
        warnings.warn("evaluate_conformal: no patient_ids, so calibration and test windows are split at random; "
                      "windows of one patient are correlated and such splits overstate the agreement",
                      UserWarning, stacklevel=2)
    dev = "cuda" if C._use_device(preds) else None
    p = _mean_probability(preds, dev)
    yy = _labels01(y)
    if len(yy) != p.numel():
        raise ValueError(f"Mismatch between prediction samples ({p.numel()}) and label samples ({len(yy)})")
    pp = _prepare(p, yy, patient_ids, cluster, mode)
    ppm = torch.as_tensor(ppm_np, dtype=torch.int32, device=p.device)
    seed = int(random_state) & 0xFFFFFFFF
    totals, counts = _split_counts(pp, seed, 0, int(n_splits), cal_thr, ppm, mode)
    totals_np, counts_np = totals.cpu().numpy().astype(np.int64), counts.cpu().numpy()
    fin = ops.finalize(counts_np)
    covered = counts_np[..., ops.COLS.index("incl0_0")] + counts_np[..., ops.COLS.index("incl1_1")]
    violated = np.where(fin["n_valid"] > 0, (covered * PPM < fin["n_valid"] * (PPM - ppm_np[None, :])).astype(np.float64),
                        np.nan)
    final: Dict = {"mode": mode, "cluster": cluster, "n_valid": int(pp["n"]), "n_splits": int(n_splits),
                   "n_units": int(len(np.unique(np.asarray(patient_ids)))) if patient_ids is not None else int(p.numel()),
                   "n_cal_mean": float(totals_np[:, :2].sum(1).mean()), "n_test_mean": float(totals_np[:, 2:].sum(1).mean())}
    for j, suf in enumerate(level_suffixes(ppm_np / PPM)):
        for m in ops.METRICS:
            mean, lo, hi = C._ci(fin[m][:, j])
            final[f"{m}{suf}"], final[f"{m}{suf}_ci_lower"], final[f"{m}{suf}_ci_upper"] = mean, lo, hi
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            final[f"coverage_violation_rate{suf}"] = float(np.nanmean(violated[:, j]))
    if make_plots:
        plot_conformal(final, ppm_np / PPM, method_name, output_dir or "./uq_plots")
    if return_details:
        return final, dict(fin, totals=totals_np, counts=counts_np, alpha_ppm=ppm_np, violated=violated)
    return final


def plot_conformal(final: Dict, alphas, uq_name: str, output_dir: str = "./uq_plots"):
    """Coverage against ``1 - alpha`` with the band over splits and the diagonal; set-type shares against alpha."""
    plt = C.plt
    if plt is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    a = np.asarray(alphas, np.float64)
    sufs = level_suffixes(a)
    order = np.argsort(a)
    fig = plt.figure(figsize=(6, 6))
    plt.plot([0, 1], [0, 1], "k--", alpha=0.5, label="Nominal")
    for key, name, style in (("coverage", "all windows", "o-"), ("coverage_class_0", "normal", "s:"),
                             ("coverage_class_1", "apnea", "^:")):
        v = np.array([final[f"{key}{sufs[j]}"] for j in order])
        plt.plot(1 - a[order], v, style, label=name)
        if key == "coverage":
            plt.fill_between(1 - a[order], [final[f"{key}{sufs[j]}_ci_lower"] for j in order],
                             [final[f"{key}{sufs[j]}_ci_upper"] for j in order], alpha=0.2)
    lo = max(0.0, float(1 - a.max()) - 0.05)
    plt.xlim(lo, 1.0)
    plt.ylim(lo, 1.0)
    plt.xlabel("Nominal coverage 1 - alpha")
    plt.ylabel("Test coverage over splits")
    plt.title(f"Conformal coverage - {uq_name}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"conformal_coverage_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)
    fig = plt.figure(figsize=(7, 5))
    for key, name in (("share_singleton", "one label"), ("share_both", "both labels"), ("share_empty", "empty")):
        plt.plot(a[order], [final[f"{key}{sufs[j]}"] for j in order], "o-", label=name)
    plt.xlabel("Miscoverage level alpha")
    plt.ylabel("Share of test windows")
    plt.title(f"Conformal set types - {uq_name}")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(os.path.join(output_dir, f"conformal_set_types_{uq_name}.png"), bbox_inches="tight")
    plt.close(fig)
