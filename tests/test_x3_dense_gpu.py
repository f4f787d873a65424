"""Dense-row mapping of the x3 layer kernels (csrc/x3_layers.hip DENSE, csrc/x3_dense_map.h) against
the whole-window-slot mapping on the same inputs: every stored element of R_l is bitwise equal (sign
bits, i.e. the dropout masks, included); the moment sums differ only in how the fp32 per-tile partials
are grouped (all terms >= 0, a partial sums <= NRT + 4 = 12 values of <= 16 rows each: <= ~2.4e-6
relative, tested with 4e-6).  End to end both mappings stay within the engine's bound of the fp32
reference model."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, rng, x3

pytestmark = pytest.mark.gpu

BOUND = 1e-5          # tests/test_x3_gpu.py: engine vs the fp32 reference, per window
MOMENT_RTOL = 4e-6
GROUPS, GRID = 2, 3   # one workgroup crosses the group change and walks several tile alignments
SENTINEL = -7.0       # rows no mapping may write keep it
SIGN_LAYERS = frozenset(int(t) for t in x3._SIGN_DEFAULT.split(","))


def _layer_case(l, n_win, variant, dev):
    """Arguments of x3_layer l (without out / stats / dense_rows) for one mask / input variant."""
    cin, cout, k = x3.CH[l], x3.CH[l + 1], x3.KS[l]
    g = torch.Generator().manual_seed(1000 * l + 10 * n_win + len(variant))
    shared = variant == "hash_shared"
    per_group = variant == "plain"            # Deep-Ensemble style: weights and BN affine per group
    n_in = n_win if shared else GROUPS * n_win
    r_in = torch.randn(n_in, 60, cin, generator=g).abs()
    sign_in, sign_out = (False, False)
    thr_in = thr_out = 0
    if variant == "hash_shared":
        thr_in, thr_out = rng.dropout_threshold(0.3), rng.dropout_threshold(0.3)
    elif variant == "sign":
        sign_in, sign_out = x3._sign(l, SIGN_LAYERS)
        thr_in, thr_out = rng.dropout_threshold(0.3), rng.dropout_threshold(0.2)
        if sign_in:  # the producer's mask travels in the sign bit (a dropped zero is -0)
            r_in = torch.where(torch.rand(r_in.shape, generator=g) < 0.3, -r_in, r_in)
            r_in[0, :, 0] = -0.0
    ng_w = GROUPS if per_group else 1
    frs, scs = zip(*[x3.pack_conv(0.05 * torch.randn(k, cin, cout, generator=g)) for _ in range(ng_w)])
    ng_a = 1 if shared else GROUPS
    sa = 10  # per-group power-of-two prescale folded into the affine, undone by gscale
    aff = torch.cat([0.5 + torch.rand(ng_a, 1, cin, generator=g), 0.3 * torch.randn(ng_a, 1, cin, generator=g)], 1)
    f32 = dict(dtype=torch.float32, device=dev)
    return dict(
        l=l, n_win=n_win, cout=cout,
        args_head=(r_in.to(**f32).contiguous(),),
        wfrag=torch.stack(frs).to(dev).contiguous(), w_gstride=(frs[0].numel() // 8 if per_group else 0),
        bias=(0.1 * torch.randn(ng_w, cout, generator=g)).to(**f32).contiguous(),
        wscale=torch.tensor(scs, **f32), p_gstride=cout if per_group else 0,
        aff=(aff * 2.0 ** sa).reshape(-1).to(**f32).contiguous(), aff_gstride=0 if shared else 2 * cin,
        gscale=torch.full((ng_a,), 2.0 ** -sa, **f32), shared=shared, thr_in=thr_in, thr_out=thr_out,
        sign_in=sign_in, sign_out=sign_out)


def _run_layer(c, dense_rows):
    o = _ext.ops()
    dev = c["wfrag"].device
    out = torch.full((GROUPS * c["n_win"] * 60 * c["cout"],), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.zeros(GROUPS * x3.STAT_SLOTS * 2 * c["cout"], dtype=torch.float64, device=dev)
    o.x3_layer(c["l"], c["args_head"][0], out, c["wfrag"], c["w_gstride"], c["bias"], c["wscale"], c["p_gstride"],
               c["aff"], c["aff_gstride"], st, c["n_win"], GROUPS, c["shared"], c["thr_in"], c["thr_out"], 12345, 7,
               500, GRID, None, None, None, c["gscale"], c["sign_in"], c["sign_out"], dense_rows)
    torch.cuda.synchronize()
    return out, st.view(GROUPS, x3.STAT_SLOTS, 2 * c["cout"]).sum(1)


@pytest.mark.parametrize("variant", ["hash_shared", "sign", "plain"])
@pytest.mark.parametrize("n_win", [67, 1])
@pytest.mark.parametrize("l", [1, 2, 3, 4])
def test_layer_dense_equals_slots(l, n_win, variant):
    """n_win 67 is past the 64-window alignment period of the 256-row tiles (32 for the 128-row ones)
    and leaves a partly filled tail tile."""
    _ext.require()
    o = _ext.ops()
    c = _layer_case(l, n_win, variant, torch.device("cuda"))
    if not o.x3_has_dense(l):
        # a layer table (csrc/x3_layers.hip, tools/probes/x3_tables/) may leave a layer's dense-row kernel
        # out (one that does not measure faster there): asking for it is then an error, not a fall-back
        with pytest.raises(RuntimeError, match="no dense-row kernel"):
            _run_layer(c, True)
        return
    out_s, mom_s = _run_layer(c, False)
    out_d, mom_d = _run_layer(c, True)
    assert not (out_s == SENTINEL).any(), "slot mapping left rows unwritten"
    assert (out_s != 0).any()
    if c["sign_out"]:
        assert (out_s.view(torch.int32) < 0).any(), "no mask in the sign bits"
    assert torch.equal(out_s.view(torch.int32), out_d.view(torch.int32)), (
        f"{(out_s.view(torch.int32) != out_d.view(torch.int32)).sum().item()} elements differ")
    err = (mom_d - mom_s).abs() / torch.maximum(mom_d.abs(), mom_s.abs()).clamp_min(1e-300)
    print(f"layer {l} n_win {n_win} {variant}: max relative moment difference {err.max().item():.3e}")
    assert (mom_s[:, c["cout"]:] > 0).any()
    assert err.max().item() <= MOMENT_RTOL


def test_dense_needs_a_batch_moment_kernel():
    """Block 6 and the per-sample-prescale kernels keep whole-window slots: asking for dense rows there
    is an error, never a silent fall-back."""
    _ext.require()
    o = _ext.ops()
    assert not o.x3_has_dense(5)
    c = _layer_case(1, 1, "plain", torch.device("cuda"))
    c["l"] = 5
    with pytest.raises(RuntimeError):
        _run_layer(c, True)


def _params(seed, dev):
    return {k: v.to(dev) for k, v in R.synthetic_params(SPEC, seed).items()}


def _x(n, seed):
    return torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(seed))


@pytest.fixture
def mappings():
    """(slot, dense) layer sets for x3.set_dense_layers; the previous choice is restored afterwards."""
    _ext.require()
    o = _ext.ops()
    prev = x3.set_dense_layers(None)
    yield (), tuple(l for l in range(1, 5) if o.x3_has_dense(l))
    x3.set_dense_layers(prev)


def test_mcd_batch_dense_equals_slots(mappings):
    dev = torch.device("cuda")
    n, T, seed, base = 67, 3, 2025, 40
    x = _x(n, 9)
    outs = []
    for layers in mappings:
        x3.set_dense_layers(layers)
        model = x3.X3Model(SPEC, [_params(13, dev)])
        outs.append(x3.mcd_batch(model, x.to(dev), T, seed=seed, pass_base=base, update_moving=False).cpu())
    assert len(mappings[1]) > 0
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"mcd_batch dense vs slot: max |dp| {d:.3e}")
    assert d <= 2e-6  # the bound of test_mcd_batch_chunked_equals_unchunked
    pc = {k: v.clone() for k, v in _params(13, "cpu").items()}
    ids = torch.arange(n)
    for t in range(T):
        r = R.forward(SPEC, pc, x, dropout=True, bn_batch_stats=True, update_moving=False, seed=seed,
                      pass_id=base + t, sample_ids=ids).reshape(-1)
        for got in outs:
            assert (got[t] - r).abs().max().item() <= BOUND


def test_deep_ensemble_dense_equals_slots(mappings):
    dev = torch.device("cuda")
    n = 67
    x = _x(n, 21)
    ps = [_params(100 + m, dev) for m in range(2)]
    outs = []
    for layers in mappings:
        x3.set_dense_layers(layers)
        outs.append(x3.forward_running(x3.X3Model(SPEC, ps), x.to(dev)).cpu())
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"forward_running (DE) dense vs slot: max |dp| {d:.3e}")
    assert d <= 1e-6
    for m in range(2):
        pc = {k: v.detach().cpu().clone() for k, v in ps[m].items()}
        r = R.forward(SPEC, pc, x).reshape(-1)
        for got in outs:
            assert (got[m, 0] - r).abs().max().item() <= BOUND
