"""Output mask of the dense-row x3 layer kernels that store it in the sign bit (x3_layer 2 and 4 = blocks
3 and 5 with ``sign_out``).  Block 5's loader waves draw it into an LDS bit table and the epilogue only
inserts the table's bits (csrc/x3_layers.hip, mask_tab_layer); block 3 hashes in its epilogue.  Either
way the stored words must equal, bit for bit, those of the slot kernel (which hashes in its epilogue),
and the sign bits must be the mask the CPU recomputes from ``ops/rng.py``.  Equality, not a tolerance;
the cases are the ones at which the table can go wrong: a workgroup that walks many tiles and crosses
the group change (one table, reused), a single partial tile, non-zero window and pass offsets (the
keys), and no dropout (no table)."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, rng, x3

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC  # both halves of the 64-bit seed reach the stream key
RATE_IN, RATE_OUT = 0.3, 0.2
SENTINEL = -7.0
CHUNKED_BOUND = 2e-6     # tests/test_x3_gpu.py::test_mcd_batch_chunked_equals_unchunked


def _case(l, n_win, groups):
    cin, cout, k = x3.CH[l], x3.CH[l + 1], x3.KS[l]
    g = torch.Generator().manual_seed(77 * l + n_win + groups)
    dev = torch.device("cuda")
    f32 = dict(dtype=torch.float32, device=dev)
    fr, sc = x3.pack_conv(0.05 * torch.randn(k, cin, cout, generator=g))
    sa = 10  # the per-group prescale folded into the affine, undone by gscale
    aff = torch.cat([0.5 + torch.rand(groups, 1, cin, generator=g), 0.3 * torch.randn(groups, 1, cin, generator=g)], 1)
    return dict(
        l=l, n_win=n_win, groups=groups, cout=cout,
        r_in=torch.randn(groups * n_win, 60, cin, generator=g).abs().to(**f32).contiguous(),
        wfrag=fr.view(1, -1).to(dev).contiguous(), bias=(0.1 * torch.randn(1, cout, generator=g)).to(**f32),
        wscale=torch.tensor([sc], **f32), aff=(aff * 2.0 ** sa).reshape(-1).to(**f32).contiguous(),
        gscale=torch.full((groups,), 2.0 ** -sa, **f32), aff_gstride=2 * cin)


def _run(c, dense_rows, grid, thr_out, pass_base, window_offset):
    o = _ext.ops()
    dev = c["wfrag"].device
    out = torch.full((c["groups"], c["n_win"], 60, c["cout"]), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.zeros(c["groups"] * x3.STAT_SLOTS * 2 * c["cout"], dtype=torch.float64, device=dev)
    # hash mask on the input (sign_in off), the block's own mask in the output's sign bit (sign_out on)
    o.x3_layer(c["l"], c["r_in"], out.view(-1), c["wfrag"], 0, c["bias"], c["wscale"], 0, c["aff"], c["aff_gstride"], st,
               c["n_win"], c["groups"], False, rng.dropout_threshold(RATE_IN), thr_out, SEED, pass_base, window_offset,
               grid, None, None, None, c["gscale"], False, True, dense_rows)
    torch.cuda.synchronize()
    return out.cpu()


def _expected_dropped(c, rate, pass_base, window_offset):
    """(groups, n_win, 60, cout) bool: the elements block l + 1's mask drops, from the host definition."""
    win = torch.arange(c["n_win"]) + window_offset
    return torch.stack([~rng.keep_mask_torch(rng.stream_key(SEED, c["l"], pass_base + g), win, 60, c["cout"], rate)
                        for g in range(c["groups"])])


# (n_win, groups, grid, pass_base, window_offset)
CASES = [
    pytest.param(67, 2, 1, 0, 0, id="67x2-one-workgroup"),     # 32 tiles per group on one table, group change
    pytest.param(67, 2, 3, 0, 0, id="67x2-three-workgroups"),  # a workgroup starts and ends inside a group
    pytest.param(1, 1, 1, 0, 0, id="one-window"),              # one partial tile
    pytest.param(3, 2, 2, 7, 500, id="offsets"),               # pass_base and window_offset in the keys
]


@pytest.mark.parametrize("n_win,groups,grid,pass_base,window_offset", CASES)
@pytest.mark.parametrize("l", [2, 4])
def test_table_mask_equals_slot_kernel_and_host_mask(l, n_win, groups, grid, pass_base, window_offset):
    _ext.require()
    assert _ext.ops().x3_has_dense(l)
    c = _case(l, n_win, groups)
    thr = rng.dropout_threshold(RATE_OUT)
    slot = _run(c, False, grid, thr, pass_base, window_offset)
    dense = _run(c, True, grid, thr, pass_base, window_offset)
    assert not (slot == SENTINEL).any() and not (dense == SENTINEL).any(), "rows left unwritten"
    si, di = slot.view(torch.int32), dense.view(torch.int32)
    sign_diff = ((si < 0) != (di < 0)).sum().item()
    mag_diff = ((si & 0x7FFFFFFF) != (di & 0x7FFFFFFF)).sum().item()
    dropped = _expected_dropped(c, RATE_OUT, pass_base, window_offset)
    host_diff = ((di < 0) != dropped).sum().item()
    print(f"layer {l} {n_win}x{groups} grid {grid}: sign bits differing from the slot kernel {sign_diff}, magnitudes "
          f"{mag_diff}, sign bits differing from the host mask {host_diff} of {dropped.numel()} "
          f"({dropped.float().mean().item():.3f} dropped)")
    assert (di & 0x7FFFFFFF).ne(0).any() and dropped.any() and not dropped.all()
    assert sign_diff == 0 and mag_diff == 0
    assert host_diff == 0


@pytest.mark.parametrize("l", [2, 4])
def test_threshold_zero_skips_the_table(l):
    """No dropout on the output: nothing is drawn, no sign bit is set, and the words equal the slot kernel's."""
    _ext.require()
    c = _case(l, 67, 2)
    slot = _run(c, False, 3, 0, 7, 500)
    dense = _run(c, True, 3, 0, 7, 500)
    assert not (dense == SENTINEL).any()
    assert torch.equal(slot.view(torch.int32), dense.view(torch.int32))
    assert not (dense.view(torch.int32) < 0).any()
    assert (dense > 0).any()


def test_mcd_batch_against_reference():
    _ext.require()
    dev = torch.device("cuda")
    n, T, seed, base = 67, 3, 2025, 40
    x = torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(9))
    model = x3.X3Model(SPEC, [{k: v.to(dev) for k, v in R.synthetic_params(SPEC, 13).items()}])
    got = x3.mcd_batch(model, x.to(dev), T, seed=seed, pass_base=base, update_moving=False).cpu()
    pc = {k: v.clone() for k, v in R.synthetic_params(SPEC, 13).items()}
    ids = torch.arange(n)
    worst = 0.0
    for t in range(T):
        r = R.forward(SPEC, pc, x, dropout=True, bn_batch_stats=True, update_moving=False, seed=seed,
                      pass_id=base + t, sample_ids=ids).reshape(-1)
        worst = max(worst, (got[t] - r).abs().max().item())
    print(f"mcd_batch vs models/reference.py, 67 windows, T = 3: max |dp| {worst:.3e} (bound {CHUNKED_BOUND:.0e})")
    assert worst <= CHUNKED_BOUND
