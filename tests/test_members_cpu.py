"""CPU: the emulation of ``ops/members.py`` against the float64 goldens of ``uq/members.py``, the identities
behind the diversity numbers, the edges, greedy selection, the cross-fit and the CLI."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import members as MB
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import members as MM
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq.recalibration import assign_folds

from . import members_fixtures as F
from .dist_utils import run_ranks

NLL = MB.MIX["nll_q"]
EXACT = [i for i in range(MB.N_MIX_COLS) if i != NLL]
ID_T, ID_N = 7, 1201


def _identity_set():
    p = np.random.RandomState(31).rand(ID_T, ID_N).astype(np.float32)
    return p, F.labels(ID_N)


# ---- emulation against golden ----
@pytest.mark.parametrize("kind", ["dyadic", "random"])
def test_pairs_eager_gives_the_golden_integers(kind):
    p, y = F.inputs(kind, 7, 1201)
    table, head = MB.pairs_eager(*F.tensors(p, y))
    gt, gh = MM.golden_member_pairs(p, y)
    assert table.dtype == torch.int64 and np.array_equal(table.numpy(), gt) and np.array_equal(head.numpy(), gh)
    assert gh[0] == 1201 - 2 - 64   # the NaN, the inf and the invalid tile


@pytest.mark.parametrize("kind", ["dyadic", "random"])
def test_mix_eager_against_golden(kind):
    p, y = F.inputs(kind, 7, 1201)
    c, fd = F.mix_counts(7, 12), F.folds(1201, 5)
    got = MB.mix_eager(*F.tensors(p, y), c, torch.from_numpy(fd), 5).numpy()
    gold = MM.golden_mix(p, y, c, fd, 5)
    assert np.array_equal(got[..., EXACT], gold[..., EXACT])
    assert np.all(np.abs(got[..., NLL] - gold[..., NLL]) <= gold[..., 0])
    assert np.array_equal(MB.mix_eager(*F.tensors(p, y), c).numpy()[..., EXACT], gold.sum(0, keepdims=True)[..., EXACT])


# ---- identities on a seeded (7, 1201) set ----
def test_brier_decomposition_identities():
    """ensemble_brier from the Gram against the float64 mean of (mean_t p - y)^2 within 1e-12: each quantised
    product is off by at most 2^-41 and the weights 1 / T^2 sum to 1, so the score moves by at most
    2^-41 = 4.5e-13, plus float64 rounding.  The ambiguity is a difference of two such scores, the second a
    mean of T."""
    p, y = _identity_set()
    div = MM.member_diversity(p, y)
    pd_ = p.astype(np.float64)
    assert abs(div["ensemble_brier"] - np.mean((pd_.mean(0) - y) ** 2)) <= 1e-12
    assert abs(div["ambiguity"] - np.mean((pd_ - pd_.mean(0)) ** 2)) <= 1e-12
    assert abs(div["mean_member_brier"] - np.mean((pd_ - y) ** 2)) <= 1e-12
    assert div["ambiguity"] > 0


def test_kw_variance_from_the_per_window_correct_counts():
    """Kohavi-Wolpert: (1 / (n T^2)) sum_w l_w (T - l_w), l_w the members correct on window w."""
    p, y = _identity_set()
    div = MM.member_diversity(p, y)
    l = ((p > 0.5) == (y != 0)).sum(0).astype(np.float64)
    assert abs(div["kw_variance"] - np.mean(l * (ID_T - l)) / ID_T ** 2) <= 1e-12


def test_pair_statistics_against_their_definitions():
    from sklearn.metrics import cohen_kappa_score, matthews_corrcoef

    p, y = _identity_set()
    div = MM.member_diversity(p, y)
    lab, right = p > 0.5, (p > 0.5) == (y != 0)
    r = p.astype(np.float64) - y
    for a, b in ((0, 1), (2, 6), (3, 3)):
        assert abs(div["kappa"][a, b] - cohen_kappa_score(lab[a], lab[b])) <= 1e-12
        assert abs(div["disagreement"][a, b] - np.mean(lab[a] != lab[b])) <= 1e-12
        assert abs(div["double_fault"][a, b] - np.mean(~right[a] & ~right[b])) <= 1e-12
        assert abs(div["error_correlation"][a, b] - matthews_corrcoef(right[a], right[b])) <= 1e-12
        assert abs(div["residual_correlation"][a, b] - np.sum(r[a] * r[b]) / np.sqrt(np.sum(r[a] ** 2) * np.sum(r[b] ** 2))) <= 1e-12
        for cls in (0, 1):
            m = y == cls
            assert abs(div[f"kappa_y{cls}"][a, b] - cohen_kappa_score(lab[a][m], lab[b][m])) <= 1e-12 or a == b
            assert abs(div[f"disagreement_y{cls}"][a, b] - np.mean(lab[a][m] != lab[b][m])) <= 1e-12
    n11, n00 = np.sum(right[0] & right[1]), np.sum(~right[0] & ~right[1])
    n10, n01 = np.sum(right[0] & ~right[1]), np.sum(~right[0] & right[1])
    assert abs(div["q_statistic"][0, 1] - (n11 * n00 - n01 * n10) / (n11 * n00 + n01 * n10)) <= 1e-12
    assert np.array_equal(div["kappa"], div["kappa"].T)


def test_subset_brier_equals_the_mix_row():
    """The Gram route quantises each product, the mixture route each window: each side is off by at most half
    a quantum per window, so the two sums differ by at most n quanta."""
    p, y = _identity_set()
    c = F.mix_counts(ID_T, 12)
    ps = MM.member_pairs(p, y)
    brier_q = MB.mix_eager(*F.tensors(p, y), c)[0, :, MB.MIX["brier_q"]].numpy()
    got = MM.subset_brier(ps, c) * ps.n_valid * MB.BRIER_SCALE
    assert np.all(np.abs(got - brier_q) <= ps.n_valid)
    assert MM.subset_brier(ps, c[3]).shape == ()


def test_member_table_against_the_definitions():
    from sklearn.metrics import brier_score_loss, log_loss

    p, y = _identity_set()
    tab = MM.member_table(p, y)
    pd_ = p.astype(np.float64)
    for t in (0, 4):
        assert abs(tab["nll"][t] - log_loss(y, np.clip(pd_[t], 1e-7, 1 - 1e-7))) <= F.NLL_TOL
        assert abs(tab["brier"][t] - brier_score_loss(y, pd_[t])) <= F.BRIER_TOL
        assert abs(tab["accuracy"][t] - np.mean((pd_[t] > 0.5) == y)) <= 1e-12
        loo = np.delete(pd_, t, 0).mean(0)
        assert abs(tab["loo_brier_delta"][t] - (np.mean((loo - y) ** 2) - np.mean((pd_.mean(0) - y) ** 2))) <= F.BRIER_TOL
    assert abs(tab["ensemble_nll"] - log_loss(y, pd_.sum(0) / ID_T)) <= F.NLL_TOL


# ---- edges ----
def test_single_member():
    p, y = _identity_set()
    div = MM.member_diversity(p[:1], y)
    assert div["disagreement"].shape == (1, 1) and all(np.isnan(div[f"mean_{k}"]) for k in MM.MEANS)
    assert np.isnan(div["kw_variance"]) and abs(div["ambiguity"]) <= 1e-12
    sel = MM.select_members(p[:1], y)
    assert sel.order.tolist() == [0] and sel.counts_path.tolist() == [[1]]
    assert np.isnan(MM.member_table(p[:1], y)["loo_nll_delta"]).all()
    res = MM.evaluate_members(p[:1], y, "one", output_dir=None)
    assert res["members_needed_nll"] == 1 and res["greedy_nll_at_1"] == res["ensemble_nll"]


def test_non_finite_window_is_dropped_everywhere():
    p, y = _identity_set()
    q = p.copy()
    q[2, 10], q[5, 11] = np.nan, -np.inf
    keep = np.ones(ID_N, bool)
    keep[[10, 11]] = False
    a, b = MB.pairs_eager(*F.tensors(q, y)), MB.pairs_eager(*F.tensors(np.ascontiguousarray(p[:, keep]), y[keep]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1][0]) == ID_N - 2
    c = F.mix_counts(ID_T, 5)
    assert torch.equal(MB.mix_eager(*F.tensors(q, y), c), MB.mix_eager(*F.tensors(np.ascontiguousarray(p[:, keep]), y[keep]), c))
    assert MM.member_table(q, y)["n_valid"] == ID_N - 2


@pytest.mark.parametrize("cls", [0, 1])
def test_single_class_gives_nan_class_tables(cls):
    p, _ = _identity_set()
    y = np.full(ID_N, cls, np.int32)
    div = MM.member_diversity(p, y)
    assert np.isnan(div[f"kappa_y{1 - cls}"]).all() and np.isnan(div[f"disagreement_y{1 - cls}"]).all()
    assert np.isfinite(div[f"disagreement_y{cls}"]).all() and np.isfinite(div["disagreement"]).all()
    tab = MM.member_table(p, y)
    assert np.isnan(tab["sensitivity" if cls == 0 else "specificity"]).all() and np.isfinite(tab["nll"]).all()
    MM.evaluate_members(p, y, "one_class", n_folds=1, n_orders=3, output_dir=None)


def test_label_rule_and_clip_at_0_half_1():
    """p = 0.5 is labelled 0 (p > 0.5, 2 s > k); p = 0 and p = 1 cost -log(1e-7) or -log(1 - 1e-7)."""
    p = np.array([[0.0, 0.5, 1.0, 0.0, 0.5, 1.0]], np.float32)
    y = np.array([0, 0, 0, 1, 1, 1], np.int32)
    table, head = MB.pairs_eager(*F.tensors(p, y))
    assert table[0, 0].tolist() == [2, 1, int(round((0.25 + 1 + 0.25 + 1) * 2 ** 40))] and head.tolist() == [6, 3]
    out = MB.mix_eager(*F.tensors(p, y), np.array([[1], [255]]))
    assert torch.equal(out[0, 0], out[0, 1])   # k = 255 of one member is that member
    hi, lo, half = -np.log(1e-7), -np.log(1 - 1e-7), -np.log(0.5)
    assert out[0, 0].tolist() == [6, 3, int(np.rint(np.array([lo, half, hi, hi, half, lo]) * 2.0 ** 36).sum()),
                                  int(2.5 * 2 ** 40), 3, 1, 2]
    assert np.array_equal(out.numpy(), MM.golden_mix(p, y, np.array([[1], [255]])))


def test_counts_with_255():
    p, y = _identity_set()
    c = np.full((2, ID_T), 255)
    c[1, ::2] = 0
    got = MB.mix_eager(*F.tensors(p, y), c).numpy()
    gold = MM.golden_mix(p, y, c)
    assert np.array_equal(got[..., EXACT], gold[..., EXACT])
    assert np.all(np.abs(got[..., NLL] - gold[..., NLL]) <= gold[..., 0])
    # 255 of every member is the plain mean up to the rounding of s: the same labels, Brier sums within n quanta
    plain = MB.mix_eager(*F.tensors(p, y), np.ones((1, ID_T), int)).numpy()[0, 0]
    assert np.array_equal(got[0, 0, 4:], plain[4:]) and abs(got[0, 0, 3] - plain[3]) <= ID_N


def test_bad_arguments_raise():
    p, y = _identity_set()
    pt, yt = F.tensors(p, y)
    ok = np.ones((1, ID_T), int)
    with pytest.raises(ValueError):
        MB.mix_eager(pt, yt, np.zeros((1, ID_T), int))
    with pytest.raises(ValueError):
        MB.mix_eager(pt, yt, np.concatenate([ok, ok * 0]))
    with pytest.raises(ValueError):
        MB.mix_eager(pt, yt, ok * 256)
    with pytest.raises(ValueError):
        MB.mix_eager(pt, yt, ok[:, :-1])
    big = torch.rand(129, 10)
    with pytest.raises(ValueError):
        MB.pairs_eager(big, torch.zeros(10))
    with pytest.raises(ValueError):
        MB.mix_eager(big, torch.zeros(10), np.ones((1, 129), int))
    with pytest.raises(ValueError):
        MM.member_diversity(big.numpy(), np.zeros(10))
    fd = torch.zeros(ID_N, dtype=torch.uint8)
    with pytest.raises(ValueError):
        MB.mix_eager(pt, yt, ok, fd, 17)
    fd[5] = 3
    with pytest.raises(ValueError):
        MB.mix_eager(pt, yt, ok, fd, 3)
    assert MB.mix_eager(pt, yt, ok, fd, 4).shape == (4, 1, 7)
    with pytest.raises(ValueError):
        MB.pairs_eager(pt, yt[:-1])
    with pytest.raises(ValueError):
        MB.pairs(pt, yt)   # the kernel entry point wants GPU tensors; it never falls back
    with pytest.raises(ValueError):
        MM.select_members(p, y, loss="auroc")
    with pytest.raises(ValueError):
        MM.select_members(p, y, k_max=ID_T + 1)


# ---- selection ----
@pytest.mark.parametrize("loss", ["nll", "brier"])
def test_greedy_selection_on_the_duplicate_fixture(loss):
    p, y, _ = F.selection_cohort()
    F.assert_selection_margins(p, y, loss, F.SEL_K, False)
    sel = MM.select_members(p, y, loss=loss, k_max=F.SEL_K)
    order, path, train = MM.golden_select(p, y, loss, F.SEL_K)
    assert np.array_equal(sel.order, order) and np.array_equal(sel.counts_path, path)
    assert np.max(np.abs(sel.train_loss - train)) <= (F.NLL_TOL if loss == "nll" else F.BRIER_TOL)
    # the best member first: members 2, 5 and 6 are the same and tie exactly, the lowest index wins
    assert sel.order[0] == F.SEL_BEST == min(F.SEL_DUPES) and sel.order[1] not in F.SEL_DUPES
    assert np.all(np.diff(sel.train_loss[:2]) < 0) and sel.subset(2) == sorted(sel.order[:2].tolist())


def test_brier_selection_through_mix_equals_greedy_on_subset_brier():
    p, y, _ = F.selection_cohort()
    F.assert_selection_margins(p, y, "brier", F.SEL_K, False)
    ps = MM.member_pairs(p, y)
    cur, order = np.zeros(F.SEL_T, int), []
    for _ in range(F.SEL_K):
        cand = [m for m in range(F.SEL_T) if cur[m] == 0]
        scores = MM.subset_brier(ps, np.stack([cur + np.eye(F.SEL_T, dtype=int)[m] for m in cand]))
        # the Gram route ties the duplicates within rounding: the lowest index among the near-minimal ones
        best = min(m for m, s in zip(cand, scores) if s <= scores.min() + 1e-12)
        cur[best] += 1
        order.append(best)
    assert MM.select_members(p, y, loss="brier", k_max=F.SEL_K).order.tolist() == order


def test_replacement_may_repeat_and_apply_has_the_path_mean():
    p, y, _ = F.selection_cohort()
    F.assert_selection_margins(p, y, "nll", F.SEL_K, True)
    sel = MM.select_members(p, y, k_max=F.SEL_K, replacement=True)
    assert np.array_equal(sel.order, MM.golden_select(p, y, "nll", F.SEL_K, True)[0])
    assert len(set(sel.order.tolist())) < F.SEL_K and sel.counts_path[-1].sum() == F.SEL_K
    for k in (1, 3, F.SEL_K):
        sub = sel.apply(p[..., None], k)
        assert sub.shape == (k, F.SEL_N, 1) and sub.dtype == np.float32
        want = (sel.counts_path[k - 1][:, None] * p.astype(np.float64)).sum(0) / k
        assert np.max(np.abs(sub[..., 0].astype(np.float64).mean(0) - want)) <= 1e-15 * k
    sub = sel.apply(torch.from_numpy(p), 2)
    assert isinstance(sub, torch.Tensor) and sub.shape == (2, F.SEL_N, 1)
    with pytest.raises(ValueError):
        sel.apply(p, F.SEL_K + 1)
    with pytest.raises(ValueError):
        sel.apply(p[:3], 1)


def test_selection_round_trips(tmp_path):
    p, y, pid = F.selection_cohort()
    for sel in (MM.select_members(p, y, k_max=3), MM.select_members(p, y, loss="brier", groups=pid, n_folds=5, seed=3)):
        path = sel.save(str(tmp_path / "sel"))
        assert path.endswith(".npz")
        back = MM.MemberSelection.load(path)
        for f in ("loss", "replacement", "n_members", "n_folds", "seed"):
            assert getattr(back, f) == getattr(sel, f)
        for f in ("order", "counts_path", "train_loss", "heldout_loss", "heldout_loss_folds", "fold_orders"):
            a, b = getattr(sel, f), getattr(back, f)
            assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True), f
        assert back.subset(2) == sel.subset(2)


# ---- cross-fit and composition ----
def test_cross_fit_paths_and_heldout_loss():
    p, y, pid = F.selection_cohort()
    codes = assign_folds(pid, 5, 2025)
    for g in np.unique(pid):
        assert len(np.unique(codes[pid == g])) == 1   # no patient in two folds
    sel = MM.select_members(p, y, groups=pid, n_folds=5, k_max=F.SEL_K)
    assert sel.fold_orders.shape == (5, F.SEL_K) and sel.heldout_loss_folds.shape == (5, F.SEL_K)
    tot_q, tot_n = np.zeros(F.SEL_K), 0
    for f in range(5):
        train = codes != f
        F.assert_selection_margins(p[:, train], y[train], "nll", F.SEL_K, False)
        alone = MM.select_members(np.ascontiguousarray(p[:, train]), y[train], k_max=F.SEL_K)
        assert np.array_equal(sel.fold_orders[f], alone.order), f
        gold = MM.golden_mix(p[:, ~train], y[~train], alone.counts_path)[0]
        assert np.max(np.abs(sel.heldout_loss_folds[f] - gold[:, 2] / 2.0 ** 36 / gold[:, 0])) <= F.NLL_TOL
        tot_q, tot_n = tot_q + gold[:, 2], tot_n + gold[0, 0]
    assert np.max(np.abs(sel.heldout_loss - tot_q / 2.0 ** 36 / tot_n)) <= F.NLL_TOL
    assert np.array_equal(sel.order, MM.select_members(p, y, k_max=F.SEL_K).order)


def test_evaluate_members_keys_and_curves(tmp_path):
    p, y, pid = F.selection_cohort()
    res = MM.evaluate_members(p, y, "fix", patient_ids=pid, n_folds=1, n_orders=30, output_dir=str(tmp_path))
    for loss in MM.LOSSES:
        assert res[f"random_{loss}_at_{F.SEL_T}_mean"] == res[f"ensemble_{loss}"] == res[f"first_{loss}_at_{F.SEL_T}"]
        assert res[f"greedy_{loss}_at_{F.SEL_T}"] == res[f"ensemble_{loss}"]
        for k in MM.default_counts(F.SEL_T):
            assert res[f"greedy_{loss}_at_{k}"] <= res[f"random_{loss}_at_{k}_mean"], (loss, k)
            assert res[f"random_{loss}_at_{k}_ci_lower"] <= res[f"random_{loss}_at_{k}_mean"] <= res[f"random_{loss}_at_{k}_ci_upper"]
        assert 1 <= res[f"members_needed_{loss}"] <= F.SEL_T
    assert res["best_member"] == F.SEL_BEST and res["ambiguity"] > 0
    assert abs(res["mean_member_brier"] - res["ambiguity"] - res["ensemble_brier"]) <= 1e-12
    for name in ("member_table_fix.csv", "member_curve_fix.csv", "member_pairwise_fix.png", "member_pruning_fix.png"):
        assert os.path.exists(tmp_path / name), name
    assert len(pd.read_csv(tmp_path / "member_table_fix.csv")) == F.SEL_T
    cross = MM.evaluate_members(p, y, "fix", patient_ids=pid, n_folds=5, n_orders=5, output_dir=None)
    assert cross["greedy_nll_at_1"] >= res["greedy_nll_at_1"] - 0.05 and cross.keys() == res.keys()
    # a huge tolerance needs one member, none needs the point from which on the path stays at the all-T loss
    assert MM.evaluate_members(p, y, "fix", n_folds=1, n_orders=2, tolerance=10.0, output_dir=None)["members_needed_nll"] == 1


def _sums_rank(rank, world):
    """Both reductions and a cross-fitted selection on this rank's shard of the windows, with the comm meter on."""
    from uncertaintyquantification_sleepapnea_1dcnn_amd.parallel import comm

    p, y, pid = F.selection_cohort()
    codes = assign_folds(pid, 5, 2025)
    meter = comm.CommMeter()
    with comm.metering(meter):
        s = MM._Sums(p, y, codes, 5)
        shard = s.p.shape[1]
        pairs = s.pairs()
        mix = s.mix(F.mix_counts(F.SEL_T, 70))
    sel = MM.select_members(p, y, groups=pid, n_folds=5, k_max=F.SEL_K)
    empty = MM._Sums(p[:, :1], y[:1]).pairs()   # one window on two ranks: rank 1 has an empty shard
    return shard, pairs, mix, meter.summary(), sel.order, sel.fold_orders, sel.heldout_loss, empty


def test_two_ranks_give_the_one_rank_integers():
    """Every rank reduces its contiguous window shard (probabilities, labels and fold codes cut alike) and the
    integer arrays travel in one all-reduce per call: both ranks hold exactly the one-rank integers."""
    p, y, pid = F.selection_cohort()
    codes = assign_folds(pid, 5, 2025)
    one = MM._Sums(p, y, codes, 5, distributed=False)
    pairs, mix = one.pairs(), one.mix(F.mix_counts(F.SEL_T, 70))
    sel = MM.select_members(p, y, groups=pid, n_folds=5, k_max=F.SEL_K)
    alone = MM._Sums(p[:, :1], y[:1], distributed=False).pairs()
    shards = []
    for shard, r_pairs, r_mix, summary, order, fold_orders, heldout, empty in run_ranks(_sums_rank, 2):
        shards.append(shard)
        assert np.array_equal(r_pairs.table, pairs.table) and r_pairs[1:] == pairs[1:]
        assert np.array_equal(r_mix, mix)
        ops = {op: v for ph in summary["phases"].values() for op, v in ph.items()}
        assert sorted(ops) == ["members_mix_all_reduce", "members_pairs_all_reduce"]
        assert ops["members_pairs_all_reduce"]["count"] == 1 and ops["members_mix_all_reduce"]["count"] == 1
        assert np.array_equal(order, sel.order) and np.array_equal(fold_orders, sel.fold_orders)
        assert np.array_equal(heldout, sel.heldout_loss)
        assert np.array_equal(empty.table, alone.table) and empty[1:] == alone[1:]
    assert sum(shards) == F.SEL_N and min(shards) > 0


def test_public_names_are_re_exported():
    from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import uq_techniques as U

    for name in ("member_table", "member_diversity", "subset_brier", "select_members", "evaluate_members", "MemberSelection"):
        assert getattr(U, name) is getattr(MM, name)


def test_cli_analyze_ensemble_members(tmp_path, capsys):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import commands

    assert "analyze_ensemble_members" in commands.COMMANDS
    p, y, pid = F.selection_cohort(n=400)
    pd.DataFrame({"True_Label": y, "Patient_ID": pid}).to_csv(tmp_path / "detail.csv", index=False)
    np.save(tmp_path / "raw.npy", p[..., None])
    table = commands.COMMANDS["analyze_ensemble_members"]([
        "--input_csv", str(tmp_path / "detail.csv"), "--raw_pred", str(tmp_path / "raw.npy"), "--folds", "3",
        "--n_orders", "5", "--output_csv", str(tmp_path / "members.csv"), "--state", str(tmp_path / "sel.npz"),
        "--output_raw_pred", str(tmp_path / "pruned.npy"), "--keep", "3", "--output_dir", str(tmp_path / "plots"),
        "--no_plots"])
    out = capsys.readouterr().out
    assert "members_needed_nll" in out and len(table) == F.SEL_T
    assert os.path.exists(tmp_path / "members.csv") and os.path.exists(tmp_path / "plots" / "member_table_detail.csv")
    assert os.path.exists(tmp_path / "plots" / "member_curve_detail.csv")
    assert np.load(tmp_path / "pruned.npy").shape == (3, 400, 1)
    sel = MM.MemberSelection.load(str(tmp_path / "sel.npz"))
    assert sel.n_folds == 3 and np.array_equal(np.load(tmp_path / "pruned.npy"), p[sel.order[:3]][..., None])
    with pytest.raises(ValueError):
        commands.COMMANDS["analyze_ensemble_members"]([
            "--input_csv", str(tmp_path / "detail.csv"), "--raw_pred", str(tmp_path / "raw.npy"), "--keep", "2"])
