"""GPU: the calibration HIP kernels (``csrc/uq_calib.hip``) against the integer emulation of
``ops/calib.py``, bit for bit, and the public API on CUDA predictions against the float64 golden."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, calib
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import calibration as C
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M

pytestmark = pytest.mark.gpu

TOL_P = 1.0 / calib.P_SCALE      # one quantum of p_q / brier_q
TOL_NLL = 1.0 / calib.NLL_SCALE  # one quantum of nll_q
SHARDS = ((0, 1000), (1000, 1001), (1001, 3001))
B = 16


def _inputs(n, n_thr, seed=1):
    """p with the exact corner values, scores with ties on the thresholds, labels, sorted thresholds."""
    rs = np.random.RandomState(seed)
    p = rs.rand(n).astype(np.float32)
    corners = np.concatenate([[0.0, 1.0, 0.5], np.arange(16, dtype=np.float32) / np.float32(15)]).astype(np.float32)
    p[:len(corners)] = corners[:n]
    s = rs.rand(n).astype(np.float32)
    thr = np.sort(s[rs.choice(n, n_thr, replace=False)]) if n_thr else np.zeros(0, np.float32)  # scores equal to a threshold
    y = (rs.rand(n) > 0.7).astype(np.int32)
    y[:2] = [1, 0]  # p = 0 with y = 1 and p = 1 with y = 0: the largest log-loss
    return torch.from_numpy(p), torch.from_numpy(s), torch.from_numpy(y), torch.from_numpy(thr.astype(np.float32))


@pytest.fixture(scope="module")
def records():
    """Device records per (n, K, J), made once and shared."""
    _ext.require()
    cache = {}

    def get(n, k, j):
        if (n, k, j) not in cache:
            p, s, y, thr = _inputs(n, j)
            cache[(n, k, j)] = calib.prep(p.cuda(), s.cuda(), y.cuda(), thr.cuda(), k)
        return cache[(n, k, j)]

    return get


@pytest.mark.parametrize("n_thr", [0, 11])
def test_calib_prep_matches_eager(n_thr):
    _ext.require()
    n, k = 3001, 15
    p, s, y, thr = _inputs(n, n_thr)
    if n_thr:
        assert int((s[:, None] == thr[None, :]).sum()) >= n_thr
    got = calib.prep(p.cuda(), s.cuda(), y.cuda(), thr.cuda(), k)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 4)
    g, r = calib.unpack(got.cpu()), calib.unpack(calib.prep_eager(p, s, y, thr, k))
    for f in ("p_q", "conf_bin", "unc_bucket", "y", "pred", "correct", "brier_q"):
        assert torch.equal(g[f], r[f]), f
    # device and host fp64 log may differ in the last bit before rint
    assert int((g["nll_q"] - r["nll_q"]).abs().max()) <= 1
    assert g["p_q"][:3].tolist() == [0, calib.P_SCALE, calib.P_SCALE // 2]
    assert g["conf_bin"][:3].tolist() == [0, k - 1, 7]
    # bin edges agree bit for bit with the float64 host rule floor(p K), also at p = fp32(i / 15)
    assert torch.equal(g["conf_bin"], torch.floor(p.double() * k).long().clamp_max(k - 1))
    assert int(g["unc_bucket"].max()) <= n_thr
    assert int(g["nll_q"].max()) > (1 << 31)  # -log(1e-7) 2^27 needs bit 31 of the word


@pytest.mark.parametrize("parity", [True, False])
@pytest.mark.parametrize("n", [70, 3001])
@pytest.mark.parametrize("k", [1, 15, 32])
@pytest.mark.parametrize("j", [0, 11, 64])
def test_calib_bootstrap_matches_eager(records, parity, n, k, j):
    rec = records(n, k, j)
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, B, 7).astype(np.int32)) if parity else None
    got = calib.bootstrap_sums(rec, B, k, j, idx=None if idx is None else idx.cuda(), seed=7)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, calib.n_columns(k, j))
    ref = calib.bootstrap_sums_eager(rec.cpu(), idx, 7, B, n, 0, k, j)
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("parity", [True, False])
def test_calib_bootstrap_invariance(records, parity):
    n, k, j = 3001, 15, 11
    rec = records(n, k, j)
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, B, 7).astype(np.int32)).cuda() if parity else None
    one = calib.bootstrap_sums(rec, B, k, j, idx=idx, seed=7, slices=1)
    for g in (1, 3, 8):  # g = 1 again: two runs are bitwise equal
        assert torch.equal(calib.bootstrap_sums(rec, B, k, j, idx=idx, seed=7, slices=g), one), g
    tot = torch.zeros_like(one)
    for lo, hi in SHARDS:
        part = calib.bootstrap_sums(rec[lo:hi].contiguous(), B, k, j, idx=idx, seed=7, n_global=n, lo=lo, slices=3)
        ref = calib.bootstrap_sums_eager(rec[lo:hi].cpu(), None if idx is None else idx.cpu(), 7, B, n, lo, k, j)
        assert torch.equal(part.cpu(), ref), (lo, hi)
        tot += part
    assert torch.equal(tot, one)


def test_calib_bootstrap_same_resamples_as_bootstrap():
    """Hash indices with the seed of ``ops.uq.bootstrap``: replicate b resamples the same windows."""
    _ext.require()
    n, k, j, seed = 3001, 15, 11, 7
    rs = np.random.RandomState(1)
    probs = torch.from_numpy(rs.rand(5, n).astype(np.float32)).cuda()
    y = torch.from_numpy((rs.rand(n) > 0.7).astype(np.int32)).cuda()
    mt = uq_ops.metrics(probs)
    s = mt[uq_ops.ENT_NATS].contiguous()
    thr = torch.from_numpy(C.coverage_thresholds(s, np.linspace(0.5, 1.0, j))).cuda()
    rec = calib.prep(mt[uq_ops.MEAN].contiguous(), s, y, thr, k)
    sums = calib.bootstrap_sums(rec, B, k, j, seed=seed)
    assert torch.equal(sums[:, 0:3 * k:3].sum(1).cpu(), torch.full((B,), n))            # bin counts
    assert torch.equal(sums[:, 3 * k:3 * k + 4 * (j + 1):4].sum(1).cpu(), torch.full((B,), n))  # bucket counts
    part = uq_ops.bootstrap_partial(mt, y, B, n, 0, seed=seed)  # column 4 = n1
    assert torch.equal(sums[:, 3 * k + 2:3 * k + 4 * (j + 1):4].sum(1).cpu(), part[:, 4].cpu().long())


def test_evaluate_calibration_on_cuda_predictions():
    _ext.require()
    n, t, k, nb, seed = 3001, 5, 15, 16, 11
    cov = np.linspace(0.5, 1.0, 11)
    rs = np.random.RandomState(1)
    probs = rs.rand(t, n).astype(np.float32)
    y = (rs.rand(n) > 0.7).astype(np.int32)
    pc = torch.from_numpy(probs).cuda()
    # the golden sees the per-window fp32 mean and entropy of the uq_reduce kernel, in float64
    mt = uq_ops.metrics(pc).cpu().numpy()
    p64, s = mt[uq_ops.MEAN].astype(np.float64), mt[uq_ops.ENT_NATS]
    thr = C.coverage_thresholds(s, cov)
    suf = C.coverage_suffixes(cov)
    for parity in (True, False):
        res = C.evaluate_calibration(pc, y, "gpu", n_bootstrap=nb, random_state=seed, parity=parity, n_bins=k,
                                     coverages=cov, make_plots=False)
        idx = M.parity_bootstrap_indices(n, nb, seed) if parity else uq_ops._hash_idx(n, nb, seed, "cpu").numpy()
        pt = {**C.golden_calibration(p64, y, k), **C.golden_selective(p64, s, y, thr)}
        rep = C.golden_replicates(p64, s, y, thr, idx, k)
        assert not any(np.isnan(v) for v in res.values())
        for key, tol in (("ece", TOL_P), ("mce", TOL_P), ("brier", TOL_P), ("nll", TOL_NLL), ("aurc", 1e-12)):
            assert abs(res[key] - pt[key]) <= tol, key
            assert abs(res[f"{key}_mean"] - np.mean(rep[key])) <= tol, key
            assert abs(res[f"{key}_ci_lower"] - np.percentile(rep[key], 2.5)) <= tol, key
            assert abs(res[f"{key}_ci_upper"] - np.percentile(rep[key], 97.5)) <= tol, key
        for jj, sfx in enumerate(suf):
            assert res[f"coverage{sfx}"] == pt["coverage"][jj]
            for key in C.CI_CURVES:  # count-derived: exact
                assert res[f"{key}{sfx}"] == pt[key][jj], (key, sfx)
                assert res[f"{key}{sfx}_mean"] == float(np.mean(rep[key][:, jj])), (key, sfx)
                assert res[f"{key}{sfx}_ci_lower"] == float(np.percentile(rep[key][:, jj], 2.5)), (key, sfx)
                assert res[f"{key}{sfx}_ci_upper"] == float(np.percentile(rep[key][:, jj], 97.5)), (key, sfx)
    cm = C.calibration_metrics(pc, y, n_bins=k)
    np.testing.assert_array_equal(cm["bin_count"], C.golden_calibration(p64, y, k)["bin_count"])
