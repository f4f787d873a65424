"""CPU: the eager emulation of the convergence sums (``ops/converge.py``) against the float64 golden of
``uq/convergence.py``, the invariances of the integer sums, and the public API, driver and CLI."""
import numpy as np
import pandas as pd
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.analysis.figures import plot_variance_convergence
from uncertaintyquantification_sleepapnea_1dcnn_amd.cli import commands
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import converge as V
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import convergence as CV
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq.drivers import convergence_from_predictions

from . import convergence_fixtures as F

FLOAT_KEYS = M.AGG_KEYS + ("mean_abs_shift",)
COUNT_KEYS = ("accuracy", "flip_rate")


@pytest.mark.parametrize("t_count", [1, 3, 50, 128])
def test_eager_matches_golden(t_count):
    """Float columns within 2e-12 of the golden (half a quantum, 4.6e-13, plus float64 evaluation error;
    measured here: at most 3.1e-14), ratios of counts exactly equal; no window is left out of the comparison."""
    p, y, orders, counts = F.random_inputs(t_count)
    F.assert_no_near_tie(p, orders, counts)
    s = F.eager("random", t_count)
    assert s.dtype == torch.int64 and tuple(s.shape) == (F.N_ORDERS + 1, len(counts), V.N_COLS)
    assert torch.all(s[..., V.COL["n_valid"]] == F.N - 1)          # the window with the NaN, in every entry
    assert torch.all(s[..., V.COL["n_y1"]] == int(np.delete(y, 3).sum()))
    got, ref = V.finalize(s), F.golden("random", t_count)
    assert set(got) == set(CV.METRICS) == set(ref)
    for k in FLOAT_KEYS:
        print(t_count, k, float(np.abs(got[k] - ref[k]).max()))
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=F.ATOL, err_msg=k)
    for k in COUNT_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    if t_count > 1:
        assert got["flip_rate"][:, 0].min() > 0.1 and got["overall_mean_variance"][:, -1].min() > 0.05


@pytest.mark.parametrize("t_count", [1, 3, 50, 128])
def test_dyadic_inputs_are_exact(t_count):
    p, y, orders, counts = F.dyadic_inputs(t_count)
    s = F.eager("dyadic", t_count)
    got, ref = V.finalize(s), F.golden("dyadic", t_count)
    for k in COUNT_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in FLOAT_KEYS:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=F.ATOL, err_msg=k)
    # k = T: the same subset in every order; exact sums give the same eleven columns
    assert torch.equal(s[:, -1], s[:1, -1].expand_as(s[:, -1]))
    assert int(s[0, -1, V.COL["flips"]]) == 0 and int(s[0, -1, V.COL["shift_q"]]) == 0
    # the tie at 0.5 is not a positive label: the constant-0.5 window is correct exactly when y = 0
    one = V.sums_eager(torch.from_numpy(p[:, 2:3].copy()), torch.from_numpy(y[2:3]), torch.from_numpy(orders), counts)
    assert torch.all(one[..., V.COL["correct"]] == int(y[2] == 0)) and torch.all(one[..., V.COL["flips"]] == 0)


def test_shards_add():
    p, y, orders, counts = F.random_inputs(50)
    pt, yt, ot = F.tensors(p, y, orders)
    parts = sum(V.sums_eager(pt[:, lo:hi].contiguous(), yt[lo:hi], ot, counts) for lo, hi in F.SHARDS)
    assert torch.equal(parts, F.eager("random", 50))


def test_limits_and_orders():
    y = torch.zeros(8, dtype=torch.int32)
    ok = (torch.rand(4, 8), y, torch.from_numpy(CV.subset_orders(4, 2, 0)), (1, 4))
    assert V.sums_eager(*ok).shape == (3, 2, V.N_COLS)
    big_t = V.MAX_T + 1
    bad = [
        (torch.rand(big_t, 8), y, torch.from_numpy(CV.subset_orders(big_t, 1, 0)), (1,)),             # T
        (ok[0], y, ok[2], tuple(range(1, V.MAX_K + 2))),                                                # K (and > T)
        (ok[0], y, torch.arange(4, dtype=torch.int32).repeat(V.MAX_R + 1, 1), (1,)),                    # R
        (ok[0], y, ok[2], (2, 1)), (ok[0], y, ok[2], (0, 1)), (ok[0], y, ok[2], (1, 5)), (ok[0], y, ok[2], ()),
        (ok[0], y[:7], ok[2], (1,)),
        (ok[0], y, torch.zeros(2, 4, dtype=torch.int32), (1,)),                                         # no permutation
        (ok[0], y, ok[2][:, :3], (1,)),
    ]
    for args in bad:
        for fn in (V.sums_eager, V.sums):       # sums checks its arguments before it asks for a GPU
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        V.sums(torch.rand(40, 8), y, torch.from_numpy(CV.subset_orders(40, 1, 0)), tuple(range(1, 34)))
    with pytest.raises(ValueError):
        V.sums(*ok, rep_groups=0)
    with pytest.raises(ValueError):
        CV.convergence_curves(np.random.rand(big_t, 8), np.zeros(8))
    o = CV.subset_orders(50, 9, 5)
    assert o.dtype == np.int32 and o.shape == (10, 50)
    np.testing.assert_array_equal(o[0], np.arange(50))
    np.testing.assert_array_equal(o, CV.subset_orders(50, 9, 5))
    rs = np.random.RandomState(5)
    np.testing.assert_array_equal(o[1:3], np.stack([rs.permutation(50), rs.permutation(50)]))
    np.testing.assert_array_equal(np.sort(o, axis=1), np.tile(np.arange(50), (10, 1)))
    assert CV.default_counts(50).tolist() == [1, 2, 3, 5, 10, 15, 20, 30, 40, 50]
    assert CV.default_counts(12).tolist() == [1, 2, 3, 5, 10, 12] and CV.default_counts(20, (5, 2)).tolist() == [2, 5, 20]
    for n in (1, 64, 16384, 1 << 20):
        for r in (1, 17, 101):
            assert 1 <= V.auto_rep_groups(n, r) <= max(1, min(8, -(-r // V.WAVES)))


def test_api_dictionary(tmp_path):
    p, y = F.spread_cohort(1500, 20)
    res = CV.evaluate_convergence(p[:, :, None], y, "unit", n_orders=24, random_state=3, output_dir=str(tmp_path))
    counts = CV.default_counts(20).tolist()
    for m in CV.METRICS:
        for k in counts:
            lo, mean, hi = (res[f"{m}_at_{k}{s}"] for s in ("_ci_lower", "_mean", "_ci_upper"))
            assert lo <= mean <= hi, (m, k)
            assert np.isfinite(res[f"{m}_at_{k}"])
        assert res[f"passes_needed_{m}"] in counts, m
    assert res["flip_rate_at_20"] == 0.0 and res["mean_abs_shift_at_20"] == 0.0
    assert res["flip_rate_at_20_ci_upper"] == 0.0 and res["mean_abs_shift_at_20_ci_upper"] == 0.0
    csv = pd.read_csv(tmp_path / "convergence_unit.csv")
    assert csv["N"].tolist() == counts
    assert {"overall_mean_variance", "overall_mean_variance_mean", "flip_rate_lower", "flip_rate_upper"} <= set(csv)
    if CV.plt is not None:
        assert (tmp_path / "convergence_unit.png").exists() and (tmp_path / "flip_rate_unit.png").exists()
    cur = CV.convergence_curves(torch.from_numpy(p), torch.from_numpy(y), n_orders=24, random_state=3)
    assert cur["counts"].tolist() == counts and cur["orders"].shape == (25, 20)
    assert cur["accuracy"].shape == (25, len(counts)) and res["accuracy_at_5"] == cur["accuracy"][0, 3]


def test_synthetic_cohort_converges():
    p, y = F.spread_cohort()
    res = CV.evaluate_convergence(p, y, "cohort", n_orders=32, random_state=1, output_dir=None, make_plots=False)
    counts = CV.default_counts(50).tolist()
    assert res["passes_needed_overall_mean_variance"] in counts

    def width(k):
        return res[f"overall_mean_variance_at_{k}_ci_upper"] - res[f"overall_mean_variance_at_{k}_ci_lower"]

    assert width(5) > width(20) > 0 and width(50) < 1e-11
    # fewer passes underestimate the ddof-0 variance, and more passes flip fewer labels
    assert res["overall_mean_variance_at_2_mean"] < res["overall_mean_variance_at_10_mean"] < res["overall_mean_variance_at_50"]
    assert res["flip_rate_at_2_mean"] > res["flip_rate_at_20_mean"] > res["flip_rate_at_50_mean"] == 0.0
    loose = CV.evaluate_convergence(p, y, "cohort", n_orders=32, random_state=1, tolerance=0.5, flip_tolerance=1.0,
                                    output_dir=None, make_plots=False)
    assert loose["passes_needed_overall_mean_variance"] <= res["passes_needed_overall_mean_variance"]
    assert loose["passes_needed_flip_rate"] == 1 and res["passes_needed_flip_rate"] > 1


def test_order_as_run_is_the_reference_curve():
    """Row 0 is what the reference's sweep would plot if each count reused the first k passes."""
    p, y = F.spread_cohort(2000, 50, seed=4)
    cur = CV.convergence_curves(p, y, n_orders=2)
    for j, k in enumerate(cur["counts"]):
        ref = np.var(p[:k].astype(np.float64), axis=0).mean()
        assert abs(cur["overall_mean_variance"][0, j] - ref) <= F.ATOL, k


def test_csv_and_cli(tmp_path):
    assert "analyze_pass_convergence" in commands.COMMANDS
    pu, yu = F.spread_cohort(1200, 20, seed=1)
    pb, yb = F.spread_cohort(700, 20, seed=2)
    out = tmp_path / "conv.csv"
    df = convergence_from_predictions(pu, yu, pb[:, :, None], yb, (5, 10, 20), str(out), n_orders=12, seed=3)
    assert list(df.columns[:3]) == ["N", "Variance_Unbalanced", "Variance_Balanced"] and df["N"].tolist() == [5, 10, 20]
    for k, vu, vb in zip(df["N"], df["Variance_Unbalanced"], df["Variance_Balanced"]):
        assert abs(vu - float(np.mean(M.per_window(pu[:k].astype(np.float64))["pred_variance"]))) <= F.ATOL
        assert abs(vb - float(np.mean(M.per_window(pb[:k].astype(np.float64))["pred_variance"]))) <= F.ATOL
    for s in ("Unbalanced", "Balanced"):
        assert (df[f"Variance_{s}_lower"] <= df[f"Variance_{s}_mean"]).all()
        assert (df[f"Variance_{s}_mean"] <= df[f"Variance_{s}_upper"]).all()
    assert plot_variance_convergence(str(out), str(tmp_path / "conv.png"), "mcd", dpi=50) == str(tmp_path / "conv.png")
    assert (tmp_path / "conv.png").exists()

    pd.DataFrame({"True_Label": yu, "Predicted_Probability": pu.mean(0)}).to_csv(tmp_path / "detail_U.csv", index=False)
    pd.DataFrame({"True_Label": yb, "Predicted_Probability": pb.mean(0)}).to_csv(tmp_path / "detail_B.csv", index=False)
    np.save(tmp_path / "raw_U.npy", pu[:, :, None])
    np.save(tmp_path / "raw_B.npy", pb)
    cli_out = tmp_path / "cli"
    t = commands.COMMANDS["analyze_pass_convergence"](
        ["--input_csv", str(tmp_path / "detail_U.csv"), "--raw_pred", str(tmp_path / "raw_U.npy"),
         "--balanced_csv", str(tmp_path / "detail_B.csv"), "--balanced_raw_pred", str(tmp_path / "raw_B.npy"),
         "--counts", "5,10", "--n_orders", "12", "--seed", "3", "--method", "de", "--output_dir", str(cli_out),
         "--no_plots"])
    assert set(t["metric"]) == set(CV.METRICS) and set(t["members_needed"]) <= {5, 10, 20}
    a = pd.read_csv(cli_out / "convergence_de.csv")
    assert a["N"].tolist() == [5, 10, 20]
    np.testing.assert_allclose(a["Variance_Unbalanced"], df["Variance_Unbalanced"], rtol=0, atol=F.ATOL)
    b = pd.read_csv(cli_out / "convergence_de_detail_U.csv")
    np.testing.assert_allclose(b["overall_mean_variance"], a["Variance_Unbalanced"], rtol=0, atol=1e-15)
    assert (cli_out / "passes_needed_de_detail_U.csv").exists()
    with pytest.raises(ValueError):
        commands.COMMANDS["analyze_pass_convergence"](
            ["--input_csv", str(tmp_path / "detail_B.csv"), "--raw_pred", str(tmp_path / "raw_U.npy"),
             "--output_dir", str(cli_out), "--no_plots"])
