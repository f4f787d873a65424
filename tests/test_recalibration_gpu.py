"""Recalibration on the GPU: ``csrc/uq_recal.hip`` against the torch float64 emulation on the same fp32 values,
bitwise invariance of the sums under the launch grid and the candidate chunking, and the public API on CUDA
predictions against the float64 goldens.

Allowances come from the emulation's own absolute term sums (``sums_eager(return_abs=True)``), never from the
kernel."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, recal
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import recalibration as RC

from . import recalibration_fixtures as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


def _dev():
    _ext.require()
    return torch.device("cuda")


def _g(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def allowance(out, absum, T):
    """``(n_valid + T + 16) 2^-52 abs_sum``: ordered summation of n_valid terms, T inner terms and a few ulps of
    exp / log / division per term."""
    return (out[..., :1] + T + 16) * U * absum


def _inputs(T, n, Q, nf, layout, kind, dev):
    p, y = F.variant(n, T, kind)
    fold = F.fold_codes(n, nf, layout) if nf > 1 else None
    return _g(p, dev), _g(y, dev), _g(fold, dev), _g(F.candidates(Q), dev)


def _within(got, ref, ab, T, what):
    got, ref, ab = (v.cpu().numpy() for v in (got, ref, ab))
    np.testing.assert_array_equal(got[..., :2], ref[..., :2], err_msg=what)
    assert np.isfinite(got).all(), what
    al = allowance(ref, ab, T)
    d = np.abs(got - ref)
    ratio = np.where(d > 0, d / np.maximum(al, 1e-300), 0.0)[..., 2:]
    print(f"{what}: max deviation / allowance {ratio.max():.3f}")
    assert ratio.max() <= 1.0, what


#        T    n      Q   F   fold codes  kind
CASES = [(1, 1, 1, 1, "grouped", "plain"),
         (1, 63, 4, 2, "shuffled", "clip"),
         (1, 257, 64, 5, "grouped", "label2"),
         (3, 64, 5, 5, "grouped", "nan"),
         (3, 65, 4, 16, "shuffled", "label2"),
         (3, 20001, 64, 1, "grouped", "plain"),
         (50, 65, 1, 2, "shuffled", "nan"),
         (50, 257, 5, 5, "grouped", "clip"),
         (50, 20001, 8, 5, "grouped", "nan"),
         (128, 257, 64, 16, "shuffled", "clip"),
         (128, 20001, 4, 2, "grouped", "label2")]


@pytest.mark.parametrize("objective", RC.OBJECTIVES)
@pytest.mark.parametrize("T,n,Q,nf,layout,kind", CASES)
def test_sums_match_emulation(T, n, Q, nf, layout, kind, objective):
    dev = _dev()
    p, y, fold, th = _inputs(T, n, Q, nf, layout, kind, dev)
    got = recal.sums(p, y, fold, th, nf, objective)
    ref, ab = recal.sums_eager(p, y, fold, th, nf, objective, return_abs=True)
    assert tuple(got.shape) == (nf, Q, 12) and got.dtype == torch.float64 and got.is_cuda
    _within(got, ref, ab, T, f"T={T} n={n} Q={Q} F={nf} {layout} {kind} {objective}")


@pytest.mark.parametrize("objective", RC.OBJECTIVES)
def test_sums_are_bitwise_invariant(objective):
    """Under the launch grid, the candidate chunking, a candidate's neighbours and the run."""
    dev = _dev()
    T, n, Q, nf = 7, 20001, 9, 5
    p, y, fold, th = _inputs(T, n, Q, nf, "grouped", "nan", dev)
    assert recal.n_ranges(n) == 79
    base = recal.sums(p, y, fold, th, nf, objective)
    for grid in (1, 3):
        assert torch.equal(recal.sums(p, y, fold, th, nf, objective, grid=grid), base), f"grid {grid}"
    assert torch.equal(recal.sums(p, y, fold, th, nf, objective), base), "run to run"
    for chunk in (1, 2, 4, 5):   # one- and two-candidate walks, every position of a candidate in its launch
        assert torch.equal(recal.sums(p, y, fold, th, nf, objective, chunk=chunk), base), f"chunk {chunk}"
    pick = [6, 2, 8]
    assert torch.equal(recal.sums(p, y, fold, th[pick].contiguous(), nf, objective), base[:, pick])
    # the planes of T = 128 leave the accumulator room for 20 candidates of 16 folds: the op chunks 64 into four
    p, y, fold, th = _inputs(128, 300, 64, 16, "shuffled", "plain", dev)
    assert recal.q_chunk(128, 16, 300) == 20
    assert torch.equal(recal.sums(p, y, fold, th, 16, objective), recal.sums(p, y, fold, th, 16, objective, chunk=7))


def test_sums_under_permutation_and_sharding():
    dev = _dev()
    T, n, Q, nf = 5, 3000, 4, 5
    p, y, fold, th = _inputs(T, n, Q, nf, "grouped", "label2", dev)
    ref, ab = recal.sums_eager(p, y, fold, th, nf, "joint", return_abs=True)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(n)).to(dev)
    shuffled = recal.sums(p[:, perm].contiguous(), y[perm], fold[perm].contiguous(), th, nf, "joint")
    _within(shuffled, ref, ab, T, "shuffled windows")
    cut = 1111
    parts = (recal.sums(p[:, :cut].contiguous(), y[:cut], fold[:cut].contiguous(), th, nf, "joint") +
             recal.sums(p[:, cut:].contiguous(), y[cut:], fold[cut:].contiguous(), th, nf, "joint"))
    _within(parts, ref, ab, T, "two shards")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 65, 20001])
@pytest.mark.parametrize("T", [1, 3])
def test_apply_matches_emulation(T, n):
    dev = _dev()
    p, _ = F.variant(n, T, "clip")
    if n >= 5:
        p[T - 1, 2] = np.nan
        p[0, n - 1] = -np.inf
    nf = 3
    fold = np.random.default_rng(n).integers(0, nf, n).astype(np.int32)
    if n >= 4:
        fold[1], fold[3] = -1, nf
    th = F.candidates(nf, seed=9)
    th[0] = (0.45, 0.3, 0.05)
    pt, ft, tt = _g(p, dev), _g(fold, dev), _g(th, dev)
    got = recal.apply(pt, ft, tt)
    ref = recal.apply_eager(pt, ft, tt)
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, n) and got.is_cuda
    g, r = got.cpu().numpy(), ref.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(g), np.isnan(r))
    bad = ~np.isfinite(p) | ((fold < 0) | (fold >= nf))[None]
    np.testing.assert_array_equal(np.isnan(g), bad)
    ok = ~bad
    assert np.max(np.abs(g[ok].astype(np.float64) - r[ok].astype(np.float64)), initial=0.0) <= 2.0 ** -24
    gold = RC.golden_apply(p, th, fold)
    assert np.max(np.abs(g[ok].astype(np.float64) - gold[ok].astype(np.float64)), initial=0.0) <= 2.0 ** -24
    assert ((g[ok] >= 0) & (g[ok] <= 1)).all()
    # one fold, no codes: the identity returns the clipped input
    ident = recal.apply(pt, None, _g(RC.IDENTITY[None], dev)).cpu().numpy()
    fin = np.isfinite(p)
    np.testing.assert_array_equal(np.isnan(ident), ~fin)
    clip = np.clip(p.astype(np.float64), 1e-7, 1 - 1e-7)
    assert np.max(np.abs(ident[fin].astype(np.float64) - clip[fin])) <= 2.0 ** -24


def test_apply_takes_an_unaligned_view():
    dev = _dev()
    p, _ = F.ensemble(130, 3)
    flat = torch.zeros(3 * 130 + 1, device=dev)
    flat[1:] = _g(p, dev).reshape(-1)
    view = flat[1:].view(3, 130)
    th = _g(np.array([[0.5, 0.4, 0.1]]), dev)
    assert torch.equal(recal.apply(view, None, th), recal.apply(_g(p, dev), None, th))


def test_binding_rejects_bad_arguments():
    dev = _dev()
    ops = torch.ops.apneauq
    p, y, _, th = _inputs(3, 70, 4, 1, "grouped", "plain", dev)
    y8 = (y != 0).to(torch.uint8)
    nofold = torch.empty(0, dtype=torch.int32, device=dev)
    fold = torch.zeros(70, dtype=torch.int32, device=dev)
    assert tuple(ops.recal_sums(p, y8, nofold, th, 1, 0, 256, 0).shape) == (1, 4, 12)
    p128, th64 = torch.zeros(128, 70, device=dev), _g(F.candidates(64), dev)
    bad = {
        "T = 129": lambda: ops.recal_sums(torch.zeros(129, 70, device=dev), y8, nofold, th, 1, 0, 256, 0),
        "Q = 65": lambda: ops.recal_sums(p, y8, nofold, _g(F.candidates(65), dev), 1, 0, 256, 0),
        "F = 17": lambda: ops.recal_sums(p, y8, fold, th, 17, 0, 256, 0),
        "no codes with F = 2": lambda: ops.recal_sums(p, y8, nofold, th, 2, 0, 256, 0),
        "fp64 probs": lambda: ops.recal_sums(p.double(), y8, nofold, th, 1, 0, 256, 0),
        "int64 labels": lambda: ops.recal_sums(p, y, nofold, th, 1, 0, 256, 0),
        "int64 fold codes": lambda: ops.recal_sums(p, y8, fold.long(), th, 1, 0, 256, 0),
        "fp32 thetas": lambda: ops.recal_sums(p, y8, nofold, th.float(), 1, 0, 256, 0),
        "objective 2": lambda: ops.recal_sums(p, y8, nofold, th, 1, 2, 256, 0),
        "range_len 0": lambda: ops.recal_sums(p, y8, nofold, th, 1, 0, 0, 0),
        "short labels": lambda: ops.recal_sums(p, y8[:69], nofold, th, 1, 0, 256, 0),
        "CPU tensors": lambda: ops.recal_sums(p.cpu(), y8.cpu(), nofold.cpu(), th.cpu(), 1, 0, 256, 0),
        "CPU labels": lambda: ops.recal_sums(p, y8.cpu(), nofold, th, 1, 0, 256, 0),
        # the planes of T = 128 leave no room for 64 candidates of 16 folds
        "LDS: T = 128, Q = 64, F = 16": lambda: ops.recal_sums(p128, y8, fold, th64, 16, 0, 256, 0),
        "apply F = 17": lambda: ops.recal_apply(p, nofold, _g(F.candidates(17), dev)),
        "apply no codes with F = 2": lambda: ops.recal_apply(p, nofold, _g(F.candidates(2), dev)),
        "apply fp64 probs": lambda: ops.recal_apply(p.double(), nofold, th),
        "apply int64 fold codes": lambda: ops.recal_apply(p, fold.long(), th),
        "apply CPU tensors": lambda: ops.recal_apply(p.cpu(), nofold.cpu(), th.cpu()),
    }
    for name, call in bad.items():
        try:
            call()
        except (RuntimeError, NotImplementedError):
            continue
        pytest.fail(f"the binding accepted: {name}")
    with pytest.raises(ValueError):
        recal.sums(p, y, None, _g(F.candidates(65), dev), 1)
    with pytest.raises(ValueError):
        recal.sums(torch.zeros(129, 70, device=dev), y, None, th, 1)
    with pytest.raises(ValueError):
        recal.sums(p, y, fold, th, 17)


@pytest.mark.parametrize("method,objective", [("temperature", "joint"), ("platt", "member"), ("beta", "joint")])
def test_fit_on_cuda_matches_golden(method, objective):
    dev = _dev()
    p, y, _ = F.fit_set()
    g = F.golden_facts(method, objective)
    pt = _g(p, dev)[..., None]
    r = RC.fit_recalibration(pt, y, method, objective)
    assert r.converged and r.n_valid == F.FIT_N and r.n_iter <= 10
    assert np.max(np.abs(r.theta - g["theta"])) <= F.theta_bound(g)
    assert abs(r.nll_after - g["nll"]) <= 1e-12
    out = r.apply(pt)
    assert isinstance(out, torch.Tensor) and out.device == pt.device and tuple(out.shape) == (F.FIT_T, F.FIT_N, 1)
    d = np.abs(out[..., 0].cpu().numpy().astype(np.float64) - RC.golden_apply(p, r.theta).astype(np.float64))
    assert d.max() <= 2.0 ** -24


def test_cross_fit_and_evaluation_on_cuda():
    dev = _dev()
    p, y, pid = F.fit_set()
    codes = F.fold_facts()
    pt = _g(p, dev)
    cal, info = RC.cross_recalibrate(pt, y, pid, F.FIT_FOLDS, "beta")
    assert isinstance(cal, torch.Tensor) and cal.is_cuda and tuple(cal.shape) == (F.FIT_T, F.FIT_N, 1)
    np.testing.assert_array_equal(info["fold"], codes)
    for f in range(F.FIT_FOLDS):
        tr = codes != f
        g = RC.golden_fit(p[:, tr], y[tr], "beta")
        assert np.linalg.eigvalsh(g["H"])[0] > 0
        assert np.max(np.abs(info["theta"][f] - g["theta"])) <= F.theta_bound(g)
    assert all(info["converged"]) and info["nll_after"] < info["nll_before"]
    gold = RC.golden_apply(p, info["theta"], codes)
    assert np.max(np.abs(cal[..., 0].cpu().numpy().astype(np.float64) - gold.astype(np.float64))) <= 2.0 ** -24
    res = RC.evaluate_recalibration(pt, y, "gpu", patient_ids=pid, n_folds=F.FIT_FOLDS, method="beta", n_bootstrap=8,
                                    random_state=3, parity=False, make_plots=False)
    # the golden on the fp32 mean prediction the analyses bin (as tests/test_calibration_*.py do)
    mean_b, mean_a = (C.per_window(x, "pred_variance", "cuda")[0].cpu().numpy().astype(np.float64) for x in (pt, cal))
    for m in RC.METRICS:
        tol = 1.0 / (2 ** 27 if m == "nll" else 2 ** 30)                # the quantisation of the integer records
        assert abs(res[f"{m}_before"] - C.golden_calibration(mean_b, y)[m]) <= tol, m
        assert abs(res[f"{m}_after"] - C.golden_calibration(mean_a, y)[m]) <= tol, m
        assert res[f"{m}_diff_ci_lower"] <= res[f"{m}_diff_ci_upper"]
    assert res["ece_after"] < res["ece_before"] and res["nll_share_improved"] == 1.0
