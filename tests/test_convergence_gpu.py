"""GPU: ``converge_kernel`` (``csrc/uq_converge.hip``) against the emulation of ``ops/converge.py``, its
invariances bit for bit, and the public API on CUDA predictions against the float64 golden."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import converge as V
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import convergence as CV

from . import convergence_fixtures as F

pytestmark = pytest.mark.gpu

INT = [V.COL[c] for c in V.INT_COLS]
QUANT = [V.COL[c] for c in V.Q_COLS]


def _kernel(p, y, orders, counts, **kw):
    return V.sums(*F.tensors(p, y, orders, "cuda"), counts, **kw)


def _assert_matches(got, ref, what=""):
    """Integer columns exactly; every quantised column within n_valid quanta per (r, k) entry: the two
    float64 evaluations of a window differ by far less than a quantum, so each window moves a sum by at
    most one."""
    assert got.dtype == torch.int64 and got.shape == ref.shape
    g = got.cpu()
    assert torch.equal(g[..., INT], ref[..., INT]), what
    n_valid = ref[..., V.COL["n_valid"]].unsqueeze(-1)
    diff = (g[..., QUANT] - ref[..., QUANT]).abs()
    print(what, "max |kernel - eager| in quanta", int(diff.max()), "with n_valid", int(n_valid.max()))
    assert torch.all(diff <= n_valid), what


@pytest.mark.parametrize("t_count", [1, 3, 50, 128])
def test_converge_kernel_matches_eager(t_count):
    """The kernel against the emulation on dyadic and on random inputs; the same launch twice is bitwise
    equal.  k = T agrees across orders within n_valid quanta and is not asserted bitwise on the random
    inputs: float64 sums of fp32 probabilities depend on the order in their last bits."""
    _ext.require()
    for kind, make in (("dyadic", F.dyadic_inputs), ("random", F.random_inputs)):
        p, y, orders, counts = make(t_count)
        if kind == "random":
            F.assert_no_near_tie(p, orders, counts)
        got = _kernel(p, y, orders, counts)
        _assert_matches(got, F.eager(kind, t_count), f"T={t_count} {kind}")
        assert torch.equal(_kernel(p, y, orders, counts), got)
        last = got[:, -1].cpu()
        assert torch.equal(last[:, INT], last[:1, INT].expand(len(last), -1))
        assert torch.all((last[:, QUANT] - last[:1, QUANT]).abs() <= last[:, :1]), kind
        if kind == "dyadic":   # exact sums: the same k = T column in every order
            assert torch.equal(last, last[:1].expand_as(last))


def test_rep_groups_and_shards_are_bitwise():
    _ext.require()
    p, y, orders, counts = F.random_inputs(50)
    whole = _kernel(p, y, orders, counts)
    for g in (1, 3, 8):
        assert torch.equal(_kernel(p, y, orders, counts, rep_groups=g), whole), g
    parts = sum(_kernel(np.ascontiguousarray(p[:, lo:hi]), y[lo:hi], orders, counts) for lo, hi in F.SHARDS)
    assert torch.equal(parts, whole)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_tile_edges(n):
    """A set that ends at, one before and one after a tile's edge: against the emulation, and bitwise the
    difference between the whole set and the rest."""
    _ext.require()
    p, y, orders, counts = F.random_inputs(50)
    head = _kernel(np.ascontiguousarray(p[:, :n]), y[:n], orders, counts)
    _assert_matches(head, V.sums_eager(*F.tensors(np.ascontiguousarray(p[:, :n]), y[:n], orders), counts), f"n={n}")
    assert torch.all(head[..., V.COL["n_valid"]] == n - (n > 3))
    rest = _kernel(np.ascontiguousarray(p[:, n:]), y[n:], orders, counts)
    assert torch.equal(head + rest, _kernel(p, y, orders, counts))


def test_single_order_single_count():
    """R = 1 (the identity only), K = 1 and counts = (T,): against the emulation, and bitwise the matching
    slice of the full launch where there is one."""
    _ext.require()
    p, y, orders, counts = F.random_inputs(50)
    whole = _kernel(p, y, orders, counts)
    for od, cs, same in ((orders[:1], counts, whole[:1]), (orders, (7,), None), (orders, (50,), whole[:, -1:]),
                         (orders[:1], (50,), whole[:1, -1:])):
        got = _kernel(p, y, od, cs)
        assert tuple(got.shape) == (len(od), len(cs), V.N_COLS)
        _assert_matches(got, V.sums_eager(*F.tensors(p, y, od), cs), f"R={len(od)} counts={cs}")
        if same is not None:
            assert torch.equal(got, same)


def test_public_api_on_cuda_predictions():
    _ext.require()
    p, y = F.spread_cohort(3001, 50, seed=3)
    p[1, 5] = np.inf
    pc = torch.from_numpy(p).cuda()
    cur = CV.convergence_curves(pc, y, n_orders=F.N_ORDERS, random_state=F.ORDER_SEED)
    F.assert_no_near_tie(p, cur["orders"], cur["counts"])
    ref = CV.golden_convergence(p, y, cur["counts"], cur["orders"])
    for k in CV.METRICS:
        print(k, float(np.abs(cur[k] - ref[k]).max()))
        np.testing.assert_allclose(cur[k], ref[k], rtol=0, atol=F.ATOL, err_msg=k)
    res = CV.evaluate_convergence(pc[:, :, None], y, "gpu", n_orders=F.N_ORDERS, random_state=F.ORDER_SEED,
                                  output_dir=None, make_plots=False)
    for m in CV.METRICS:
        for j, k in enumerate(cur["counts"]):
            assert abs(res[f"{m}_at_{k}"] - ref[m][0, j]) <= F.ATOL, (m, k)
            assert abs(res[f"{m}_at_{k}_ci_lower"] - np.percentile(ref[m][1:, j], 2.5)) <= F.ATOL, (m, k)
            assert abs(res[f"{m}_at_{k}_ci_upper"] - np.percentile(ref[m][1:, j], 97.5)) <= F.ATOL, (m, k)
            assert abs(res[f"{m}_at_{k}_mean"] - ref[m][1:, j].mean()) <= F.ATOL, (m, k)
    with pytest.raises(ValueError):
        CV.convergence_curves(torch.rand(129, 16, device="cuda"), np.zeros(16))
    with pytest.raises(RuntimeError):
        torch.ops.apneauq.converge(torch.rand(129, 16, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda"),
                                   torch.arange(129, dtype=torch.int32, device="cuda")[None],
                                   torch.ones(1, dtype=torch.int32, device="cuda"), 1)
