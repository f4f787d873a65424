"""GPU: the rank-statistics HIP kernels (``csrc/uq_rank.hip``) against the integer emulation of ``ops/rank.py``,
and the public API on CUDA predictions against scikit-learn / SciPy on the literal resamples."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, rank
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import discrimination as D
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M

from .rank_fixtures import STRUCTURES, TOL_PR, TOL_RANK, check_against_golden, make_scores

pytestmark = pytest.mark.gpu

B = 16
ULPS = 2.0 ** -50   # per non-empty group: a few fp64 ulps of a term of at most 1, before and after quantisation


@pytest.fixture(scope="module")
def prepared():
    """Device prep per (n, structure), made once and shared."""
    _ext.require()
    cache = {}

    def get(n, structure):
        if (n, structure) not in cache:
            s, y = make_scores(n, structure)
            cache[(n, structure)] = rank.prep(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())
        return cache[(n, structure)]

    return get


def check_scan(w, packed, splits=0):
    """Kernel sums of the weight rows against the emulation: integers bit for bit, PR terms within ULPS per group."""
    got = rank.scan_sums(w, packed, splits=splits).cpu()
    ref = rank.scan_sums_eager(w.cpu().contiguous(), packed.cpu())
    assert got.dtype == torch.int64 and tuple(got.shape) == (w.shape[0], 6)
    assert torch.equal(got[:, :4], ref[:, :4])
    fg, fr = rank.finalize(got), rank.finalize(ref)
    for k in ("pr_auc", "average_precision"):
        assert np.array_equal(np.isnan(fg[k]), np.isnan(fr[k])), k
        err = np.nan_to_num(np.abs(fg[k] - fr[k]))
        print(f"{k}: max |kernel - emulation| {err.max():.3e}, bound per group {ULPS:.3e}")
        assert np.all(err <= fr["groups"] * ULPS), k
    return got


@pytest.mark.parametrize("parity", [True, False])
@pytest.mark.parametrize("n", [70, 3001])
def test_rank_count_matches_eager(prepared, parity, n):
    pr = prepared(n, "levels8")
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, B, 7).astype(np.int32)) if parity else None
    got = rank.weights(pr["pos"], n, B, None if idx is None else idx.cuda(), seed=7)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, n) and got.stride(0) % 4 == 0
    assert torch.equal(got.cpu(), rank.weights_eager(pr["pos"].cpu(), n, B, idx, 7))
    part = rank.weights(pr["pos"], n, 5, None if idx is None else idx[4:9].cuda(), seed=7, b0=4)  # a later chunk
    assert torch.equal(part, got[4:9])


def test_rank_count_skips_out_of_range_and_dropped(prepared):
    n = 257
    s, y = make_scores(n, "continuous")
    s[[3, 50]] = np.nan
    pr = rank.prep(torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda())
    idx = M.parity_bootstrap_indices(n, B, 2).astype(np.int32)
    idx[0, :3] = [-1, n, 3]
    got = rank.weights(pr["pos"], n - 2, B, torch.from_numpy(idx).cuda())
    assert torch.equal(got.cpu(), rank.weights_eager(pr["pos"].cpu(), n - 2, B, torch.from_numpy(idx)))
    check_scan(got, pr["packed"])


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("n", [70, 257, 3001])
def test_rank_scan_matches_eager(prepared, n, structure):
    pr = prepared(n, structure)
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, B, 7).astype(np.int32)).cuda()
    w = rank.weights(pr["pos"], n, B, idx)
    assert bool((w == 0).any())  # bootstrap weights contain zeros
    got = check_scan(w, pr["packed"])
    if structure == "equal":   # one tie group covers the whole range of every workgroup
        assert np.all(rank.finalize(got)["auroc"] == 0.5)
        assert torch.equal(check_scan(w, pr["packed"], splits=8), got)


def test_rank_scan_special_weights(prepared):
    n = 3001
    pr = prepared(n, "levels8")
    rs = np.random.RandomState(4)
    z = (pr["packed"].cpu().numpy() & 1).astype(bool)
    w = rs.randint(0, 1001, size=(6, n)).astype(np.int32)   # cluster-style weights up to 1000
    w[1, rs.rand(n) < 0.5] = 0
    w[2, z] = 0             # no positives
    w[3, ~z] = 0            # no negatives
    w[4] = 0                # nothing drawn
    w[5, :] = 0
    w[5, [0, n - 1]] = 1000
    got = check_scan(torch.from_numpy(w).cuda(), pr["packed"])
    fin = rank.finalize(got)
    assert np.isnan(fin["auroc"][2:5]).all() and not np.isnan(fin["auroc"][[0, 1, 5]]).any()
    assert got[4].tolist() == [0] * 6 and int(got[2, 1]) == 0 and int(got[3, 0]) == int(got[3, 1]) > 0
    # a (B, n) tensor with unaligned rows is copied to aligned rows by the binding
    assert torch.equal(rank.scan_sums(torch.from_numpy(w).cuda()[:, 1:], pr["packed"][1:].clone() | rank.START_BIT).cpu(),
                       rank.scan_sums_eager(torch.from_numpy(w[:, 1:]).contiguous(),
                                            (pr["packed"][1:].clone() | rank.START_BIT).cpu()))


def test_rank_scan_grid_invariance(prepared):
    n = 3001
    pr = prepared(n, "levels8")   # 8 levels: a tie group lies across every nominal split point
    b8 = rank.split_bounds(pr["packed"], 8).cpu().numpy()
    assert np.all(b8[1:-1] != (np.arange(1, 8) * n) // 8)
    idx = torch.from_numpy(M.parity_bootstrap_indices(n, B, 7).astype(np.int32)).cuda()
    w = rank.weights(pr["pos"], n, B, idx)
    one = rank.scan_sums(w, pr["packed"], splits=1)
    for g in (1, 2, 8, 64):   # g = 1 again: two runs are bitwise equal
        assert torch.equal(rank.scan_sums(w, pr["packed"], splits=g), one), g
    pc = prepared(n, "continuous")
    wc = rank.weights(pc["pos"], n, B, idx)
    onec = rank.scan_sums(wc, pc["packed"], splits=1)
    for g in (2, 8):
        assert torch.equal(rank.scan_sums(wc, pc["packed"], splits=g), onec), g


def test_public_api_on_cuda_predictions():
    _ext.require()
    n, t, seed = 3001, 8, 11
    rs = np.random.RandomState(1)
    y = (rs.rand(n) > 0.7).astype(np.int32)
    probs = np.clip(rs.rand(t, n) * 0.8 + 0.25 * y[None] * rs.rand(t, n), 0, 1).astype(np.float32)
    pids = np.repeat(np.arange(12), [40, 310, 75, 5, 160, 90, 220, 130, 61, 180, 29, 1701])
    pc = torch.from_numpy(probs).cuda()
    # the golden sees the per-window fp32 mean and entropy of the uq_reduce kernel, in float64
    mt = uq_ops.metrics(pc).cpu().numpy()
    p64, ent = mt[uq_ops.MEAN].astype(np.float64), mt[uq_ops.ENT_NATS].astype(np.float64)
    wrong = ((mt[uq_ops.MEAN] > 0.5).astype(np.int32) != y).astype(np.int32)
    uniq = np.unique(pids)
    win = [np.flatnonzero(pids == u) for u in uniq]
    for cluster in (False, True):
        if cluster:
            draws = M.parity_bootstrap_indices(len(uniq), B, seed)
            idx = [np.concatenate([win[d] for d in row]) for row in draws]
        else:
            idx = list(M.parity_bootstrap_indices(n, B, seed))
        res = D.evaluate_discrimination(pc, y, "gpu", n_bootstrap=B, random_state=seed, make_plots=False,
                                        patient_ids=pids if cluster else None)
        for task, s, tg in (("apnea", p64, y), ("error", ent, wrong)):
            pt = D.golden_discrimination(s, tg)
            rows = [D.golden_discrimination(s[ix], tg[ix]) for ix in idx]
            rep = {k: np.array([r[k] for r in rows]) for k in rows[0]}
            got = D.discrimination_replicates(pc, y, task=task, n_bootstrap=B, random_state=seed,
                                              patient_ids=pids if cluster else None)
            check_against_golden(got, rep)
            for k, tol in (("auroc", TOL_RANK), ("u_statistic", TOL_RANK), ("pr_auc", TOL_PR), ("average_precision", TOL_PR)):
                assert abs(res[f"{task}_{k}"] - pt[k]) <= tol, (task, k)
                assert abs(res[f"{task}_{k}_mean"] - np.mean(rep[k])) <= tol * max(1.0, abs(np.mean(rep[k]))), (task, k)
                assert abs(res[f"{task}_{k}_ci_lower"] - np.percentile(rep[k], 2.5)) <= tol, (task, k)
                assert abs(res[f"{task}_{k}_ci_upper"] - np.percentile(rep[k], 97.5)) <= tol, (task, k)
            assert abs(res[f"{task}_p_value"] - pt["p_value"]) <= 1e-12 * pt["p_value"]
    # hash draws: the resamples of the other analyses for the same seed
    hidx = uq_ops._hash_idx(n, B, seed, "cpu").numpy()
    got = D.discrimination_replicates(pc, y, task="apnea", n_bootstrap=B, random_state=seed, parity=False)
    check_against_golden(got, D.golden_replicates(p64, y, hidx))


def test_binding_limits_raise(prepared):
    pr = prepared(70, "levels8")
    ops = _ext.ops()
    w = torch.ones(2, 70, dtype=torch.int32, device="cuda")
    bounds = rank.split_bounds(pr["packed"], 1)
    with pytest.raises(RuntimeError):
        ops.rank_scan(w.long(), pr["packed"], bounds)
    with pytest.raises(RuntimeError):
        ops.rank_scan(w, pr["packed"][:69], bounds)
    with pytest.raises(RuntimeError):
        ops.rank_scan(w, pr["packed"], torch.zeros(rank.MAX_SPLITS + 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.rank_scan(w.cpu(), pr["packed"], bounds)
    big = w.clone()
    big[0, :2] = 1 << 30   # total weight 2^31
    with pytest.raises(RuntimeError):
        ops.rank_scan(big, pr["packed"], bounds)
    with pytest.raises(ValueError):
        rank.scan_sums(big, pr["packed"])
    big[0, 0] = -1
    with pytest.raises(ValueError):
        rank.scan_sums(big, pr["packed"])
    with pytest.raises(RuntimeError):
        ops.rank_count(pr["pos"].long(), None, 0, 0, 2, 70)
    with pytest.raises(RuntimeError):
        ops.rank_count(pr["pos"], None, 0, 0, 2, 71)
    with pytest.raises(RuntimeError):
        ops.rank_count(pr["pos"], torch.zeros(2, 69, dtype=torch.int32, device="cuda"), 0, 0, 2, 70)
    with pytest.raises(RuntimeError):   # more than 2^27 windows (a zero-stride view: no memory behind it)
        ops.rank_count(torch.zeros(1, dtype=torch.int32, device="cuda").expand(rank.MAX_N + 1), None, 0, 0, 1, 1)
    # out-of-range split points are clamped by the kernel: the result is that of the clamped bounds
    wild = torch.tensor([-5, 1 << 30], dtype=torch.int32, device="cuda")
    assert torch.equal(ops.rank_scan(w, pr["packed"], wild), ops.rank_scan(w, pr["packed"], bounds))
