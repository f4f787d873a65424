"""GPU: ``member_pairs_kernel`` and ``member_mix_kernel`` (``csrc/uq_members.hip``) against the emulation of
``ops/members.py`` integer for integer, their invariances bit for bit, the binding's limits, and the public
API on CUDA predictions against the float64 goldens."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import members as MB
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import members as MM

from . import members_fixtures as F

pytestmark = pytest.mark.gpu

# the pair matrix is cut into 4 x 4 patches, 256 / slices of them per workgroup: T = 1, 2, 3 are one ragged patch
# (64 slices), 50 is ragged (2 slices), 64 an exact multiple of the patch, 65 one more; 88 fills one workgroup
# with 253 patches, 89 needs a second, 128 three
T_SET = [1, 2, 3, 50, 64, 65, 88, 89, 128]
NLL = MB.MIX["nll_q"]
EXACT = [i for i in range(MB.N_MIX_COLS) if i != NLL]


def _pairs(p, y, **kw):
    return MB.pairs(*F.tensors(p, y, "cuda"), **kw)


def _mix(p, y, counts, fold=None, n_folds=1, **kw):
    fd = None if fold is None else torch.from_numpy(np.asarray(fold)).cuda()
    return MB.mix(*F.tensors(p, y, "cuda"), counts, fd, n_folds, **kw)


def _assert_pairs(got, ref, what=""):
    for g, r in zip(got, ref):
        assert g.dtype == torch.int64 and g.shape == r.shape
        assert torch.equal(g.cpu(), r), what


def _assert_mix(got, ref, what=""):
    """Every column but nll_q exactly; nll_q within n_valid quanta per (fold, row): the two float64 logarithms of
    a window differ by far less than a quantum, so each window moves a sum by at most one."""
    assert got.dtype == torch.int64 and got.shape == ref.shape
    g = got.cpu()
    assert torch.equal(g[..., EXACT], ref[..., EXACT]), what
    diff = (g[..., NLL] - ref[..., NLL]).abs()
    print(what, "max |kernel - eager| of nll_q in quanta", int(diff.max()), "with n_valid", int(ref[..., 0].max()))
    assert torch.all(diff <= ref[..., 0]), what


@pytest.mark.parametrize("t_count", T_SET)
def test_pairs_kernel_matches_eager(t_count):
    """Dyadic and random probabilities with a NaN, an inf and a whole invalid tile: the same integers as the
    emulation, symmetric, and the same launch twice is bitwise equal."""
    _ext.require()
    for kind in ("dyadic", "random"):
        p, y = F.inputs(kind, t_count)
        got = _pairs(p, y)
        _assert_pairs(got, F.eager_pairs(kind, t_count), f"T={t_count} {kind}")
        assert torch.equal(got[0], got[0].transpose(0, 1))
        again = _pairs(p, y)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pairs_tile_edges(n):
    """A set that ends at, one before and one after a tile's edge: against the emulation, and bitwise the
    difference between the whole set and the rest."""
    _ext.require()
    p, y = F.random_inputs(50)
    head = _pairs(np.ascontiguousarray(p[:, :n]), y[:n])
    _assert_pairs(head, MB.pairs_eager(*F.tensors(np.ascontiguousarray(p[:, :n]), y[:n])), f"n={n}")
    assert int(head[1][0]) == n - (n > 3)
    rest = _pairs(np.ascontiguousarray(p[:, n:]), y[n:])
    whole = _pairs(p, y)
    assert torch.equal(head[0] + rest[0], whole[0]) and torch.equal(head[1] + rest[1], whole[1])


@pytest.mark.parametrize("t_count", T_SET)
def test_mix_kernel_matches_eager(t_count):
    """Six rows, among them k = 1, k = T and k = 255 T, without fold codes."""
    _ext.require()
    for kind in ("dyadic", "random"):
        p, y = F.inputs(kind, t_count)
        got = _mix(p, y, F.mix_counts(t_count, 6))
        _assert_mix(got, F.eager_mix(kind, t_count, 6, 0), f"T={t_count} {kind}")
        assert torch.equal(_mix(p, y, F.mix_counts(t_count, 6)), got)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_mix_tile_edges(n):
    _ext.require()
    p, y = F.random_inputs(50)
    c = F.mix_counts(50, 6)
    head = _mix(np.ascontiguousarray(p[:, :n]), y[:n], c)
    _assert_mix(head, MB.mix_eager(*F.tensors(np.ascontiguousarray(p[:, :n]), y[:n]), c), f"n={n}")
    assert torch.all(head[..., 0] == n - (n > 3))
    assert torch.equal(head + _mix(np.ascontiguousarray(p[:, n:]), y[n:], c), _mix(p, y, c))


def test_mix_rows_do_not_depend_on_their_chunk():
    """Q = 130 is three launches; a row's sums are bitwise the same alone, in a shorter set of rows and there."""
    _ext.require()
    p, y = F.random_inputs(50)
    c = F.mix_counts(50, 130)
    full = _mix(p, y, c)
    _assert_mix(full, F.eager_mix("random", 50, 130, 0), "Q=130")
    for q in (1, 64, 65):
        assert torch.equal(_mix(p, y, c[:q]), full[:, :q]), q
    for q in (0, 63, 64, 129):
        assert torch.equal(_mix(p, y, c[q:q + 1]), full[:, q:q + 1]), q
    assert torch.equal(_mix(p, y, c[60:70]), full[:, 60:70])


@pytest.mark.parametrize("n_folds", [1, 5, 16])
def test_mix_folds(n_folds):
    """Fold codes in runs, the last fold empty (F > 1): against the emulation; the folds add up to the sums
    without folds, and no codes are fold 0 of F = 1."""
    _ext.require()
    p, y = F.random_inputs(50)
    c = F.mix_counts(50, 9)
    fd = F.folds(F.N, n_folds)
    got = _mix(p, y, c, fd, n_folds)
    _assert_mix(got, F.eager_mix("random", 50, 9, n_folds), f"F={n_folds}")
    if n_folds > 1:
        assert torch.all(got[n_folds - 1] == 0) and torch.all(got[0, :, 0] > 0)
    plain = _mix(p, y, c)
    assert torch.equal(got.sum(0, keepdim=True), plain)
    assert torch.equal(_mix(p, y, c, np.zeros(F.N, np.uint8), 1), plain)


def test_launch_shape_shards_and_permutation_are_bitwise():
    _ext.require()
    p, y = F.random_inputs(50)
    c = F.mix_counts(50, 9)
    fd = F.folds(F.N, 5)
    pw, mw = _pairs(p, y), _mix(p, y, c, fd, 5)
    for g in (1, 7, 500):
        got = _pairs(p, y, grid=g)
        assert torch.equal(got[0], pw[0]) and torch.equal(got[1], pw[1]), g
        assert torch.equal(_mix(p, y, c, fd, 5, grid=g), mw), g
    for s in (1, 8, 64):
        got = _pairs(p, y, slices=s, grid=3)
        assert torch.equal(got[0], pw[0]) and torch.equal(got[1], pw[1]), s
    cut = lambda lo, hi: (np.ascontiguousarray(p[:, lo:hi]), y[lo:hi])   # noqa: E731
    parts = [_pairs(*cut(lo, hi)) for lo, hi in F.SHARDS]
    assert torch.equal(sum(t for t, _ in parts), pw[0]) and torch.equal(sum(h for _, h in parts), pw[1])
    assert torch.equal(sum(_mix(*cut(lo, hi), c, fd[lo:hi], 5) for lo, hi in F.SHARDS), mw)
    perm = np.random.RandomState(4).permutation(F.N)
    got = _pairs(np.ascontiguousarray(p[:, perm]), y[perm])
    assert torch.equal(got[0], pw[0]) and torch.equal(got[1], pw[1])
    assert torch.equal(_mix(np.ascontiguousarray(p[:, perm]), y[perm], c, fd[perm], 5), mw)


def test_limits_raise_from_the_binding():
    """Each of these is rejected by a check of the binding, before anything is launched."""
    _ext.require()
    ops = _ext.ops()
    p, y = (t.cuda() for t in F.tensors(*F.random_inputs(8, 256)))
    y = y.to(torch.int32)
    c = torch.ones(3, 8, dtype=torch.int32)   # the counts travel as a host tensor
    fd = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert ops.member_pairs(p, y, 0, 0)[0].shape == (8, 8, 3) and ops.member_mix(p, y, fd, c, 2, 0).shape == (2, 3, 7)
    big = torch.rand(129, 256, device="cuda")
    bad = [lambda: ops.member_pairs(big, y, 0, 0),
           lambda: ops.member_mix(big, y, None, torch.ones(1, 129, dtype=torch.int32), 1, 0),
           lambda: ops.member_mix(p, y, None, torch.ones(65, 8, dtype=torch.int32), 1, 0),
           lambda: ops.member_mix(p, y, fd, c, 17, 0),
           lambda: ops.member_pairs(p.t().contiguous().t(), y, 0, 0),          # not contiguous
           lambda: ops.member_mix(p.t().contiguous().t(), y, None, c, 1, 0),
           lambda: ops.member_mix(p, y, None, c.t().contiguous().t(), 1, 0),
           lambda: ops.member_pairs(p.cpu(), y.cpu(), 0, 0),                   # not on the GPU
           lambda: ops.member_pairs(p, y.cpu(), 0, 0),
           lambda: ops.member_mix(p, y, fd.cpu(), c, 2, 0),
           lambda: ops.member_mix(p, y, None, c.cuda(), 1, 0),                 # the counts must be on the host
           lambda: ops.member_pairs(p.double(), y, 0, 0),                      # wrong dtype
           lambda: ops.member_pairs(p, y.long(), 0, 0),
           lambda: ops.member_mix(p, y, fd.int(), c, 2, 0),
           lambda: ops.member_mix(p, y, None, c.long(), 1, 0),
           lambda: ops.member_mix(p, y, None, c * 0, 1, 0),                    # a row of zeros
           lambda: ops.member_mix(p, y, None, c * 256, 1, 0),                  # a count above 255
           lambda: ops.member_pairs(p, y, 0, 3),                               # slices not a power of two
           lambda: ops.member_pairs(p, y[:255], 0, 0)]
    for i, call in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
            pytest.fail(f"case {i} did not raise")


# ---- the public API on CUDA predictions ----
API_T, API_N = 50, 3001


def _api_inputs():
    p = np.random.RandomState(21).rand(API_T, API_N).astype(np.float32)
    p[7, 100] = np.inf
    return p, F.labels(API_N)


def _direct_member_table(p, y):
    """Float64 NumPy from the definitions, member by member."""
    ok = np.isfinite(p).all(0)
    p, y = p[:, ok].astype(np.float64), y[ok] != 0

    def losses(m):
        pt = np.clip(np.where(y, m, 1 - m), 1e-7, 1 - 1e-7)
        return float(np.mean(-np.log(pt))), float(np.mean((m - y) ** 2))

    out = {k: [] for k in ("accuracy", "sensitivity", "specificity", "nll", "brier", "loo_nll_delta", "loo_brier_delta")}
    full = losses(p.sum(0) / len(p))
    for t in range(len(p)):
        lab = p[t] > 0.5
        out["accuracy"].append(np.mean(lab == y))
        out["sensitivity"].append(np.mean(lab[y]))
        out["specificity"].append(np.mean(~lab[~y]))
        nll, brier = losses(p[t])
        loo = losses(np.delete(p, t, 0).sum(0) / (len(p) - 1))
        out["nll"].append(nll)
        out["brier"].append(brier)
        out["loo_nll_delta"].append(loo[0] - full[0])
        out["loo_brier_delta"].append(loo[1] - full[1])
    return {k: np.array(v) for k, v in out.items()}, full


def test_member_table_and_diversity_on_cuda():
    _ext.require()
    from sklearn.metrics import brier_score_loss, cohen_kappa_score, log_loss

    p, y = _api_inputs()
    pc = torch.from_numpy(p).cuda()
    tab = MM.member_table(pc, y)
    ref, full = _direct_member_table(p, y)
    for k in ("accuracy", "sensitivity", "specificity"):
        assert np.max(np.abs(tab[k] - ref[k])) <= F.COUNT_TOL, k
    # a term is rounded by at most half a quantum, so a mean is within half a quantum and a delta of two within one
    for k, tol in (("nll", F.NLL_TOL), ("brier", F.BRIER_TOL), ("loo_nll_delta", F.NLL_TOL), ("loo_brier_delta", F.BRIER_TOL)):
        print(k, np.max(np.abs(tab[k] - ref[k])), tol)
        assert np.max(np.abs(tab[k] - ref[k])) <= tol, k
    assert abs(tab["ensemble_nll"] - full[0]) <= F.NLL_TOL and abs(tab["ensemble_brier"] - full[1]) <= F.BRIER_TOL
    ok = np.isfinite(p).all(0)
    pv, yv = p[:, ok].astype(np.float64), y[ok]
    assert abs(tab["nll"][3] - log_loss(yv, np.clip(pv[3], 1e-7, 1 - 1e-7))) <= F.NLL_TOL
    assert abs(tab["brier"][3] - brier_score_loss(yv, pv[3])) <= F.BRIER_TOL

    div = MM.member_diversity(pc, y)
    gt, gh = MM.golden_member_pairs(p, y)
    gold = MM._diversity(MM.PairSums(gt, int(gh[0]), int(gh[1])))
    for k, v in gold.items():
        tol = F.BRIER_TOL if ("brier" in k or k in ("ambiguity", "gram")) else F.COUNT_TOL
        assert np.allclose(div[k], v, rtol=0, atol=tol, equal_nan=True), k
    assert abs(div["kappa"][4, 9] - cohen_kappa_score(pv[4] > 0.5, pv[9] > 0.5)) <= F.COUNT_TOL
    assert abs(div["ensemble_brier"] - np.mean((pv.mean(0) - yv) ** 2)) <= F.BRIER_TOL
    assert abs(div["ambiguity"] - np.mean((pv - pv.mean(0)) ** 2)) <= F.BRIER_TOL
    assert abs(div["disagreement"][4, 9] - np.mean((pv[4] > 0.5) != (pv[9] > 0.5))) <= F.COUNT_TOL


@pytest.mark.parametrize("loss", ["nll", "brier"])
@pytest.mark.parametrize("replacement", [False, True])
def test_select_members_on_cuda_equals_golden(loss, replacement):
    _ext.require()
    p, y, _ = F.selection_cohort()
    F.assert_selection_margins(p, y, loss, F.SEL_K, replacement)
    order, path, train = MM.golden_select(p, y, loss, F.SEL_K, replacement)
    sel = MM.select_members(torch.from_numpy(p).cuda(), y, loss=loss, k_max=F.SEL_K, replacement=replacement)
    assert np.array_equal(sel.order, order) and np.array_equal(sel.counts_path, path)
    assert np.max(np.abs(sel.train_loss - train)) <= (F.NLL_TOL if loss == "nll" else F.BRIER_TOL)


def test_evaluate_members_on_cuda_equals_cpu():
    """The same call on CUDA predictions and on their CPU copy, on the cohort whose every greedy step (whole
    paths, all windows and each fold's complement) is margin-checked, so the orders cannot hinge on the quanta by
    which the two NLL sums may differ: every key that comes from integers both sides compute identically is
    equal; the NLL keys are within one quantum of the mean."""
    _ext.require()
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq.recalibration import assign_folds

    p, y, pid = F.selection_cohort()
    p = p.copy()
    p[3, 100] = np.inf
    codes = assign_folds(pid, 3, 2025)
    for loss in MM.LOSSES:
        for f in (None, 0, 1, 2):
            train = np.isfinite(p).all(0) & (np.ones(len(y), bool) if f is None else codes != f)
            F.assert_selection_margins(p[:, train], y[train], loss, F.SEL_T, False)
    kw = dict(patient_ids=pid, n_folds=3, n_orders=20, output_dir=None, make_plots=False)
    dev = MM.evaluate_members(torch.from_numpy(p).cuda(), y, "cuda", **kw)
    cpu = MM.evaluate_members(p, y, "cpu", **kw)
    assert dev.keys() == cpu.keys()
    for k, v in cpu.items():
        if isinstance(v, str) or "needed" in k or k in ("best_member", "worst_member"):
            assert dev[k] == v, k
        elif "nll" in k:
            assert abs(dev[k] - v) <= F.NLL_TOL, (k, dev[k], v)
        else:
            assert dev[k] == v or (np.isnan(dev[k]) and np.isnan(v)), (k, dev[k], v)
