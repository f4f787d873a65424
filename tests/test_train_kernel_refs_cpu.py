"""The float64 oracle of the dedicated training kernels (``tests/train_kernel_refs.py``) checked where no GPU
is needed:

* composed into one whole training step (n = 6, every internal rounding switched off), the per-kernel
  references reproduce float64 autograd over ``models/reference.py:forward`` (same masks) to 1e-9: logits,
  loss, every gradient, the moving statistics;
* every allowance is far below the effect of a real mistake -- a dropped row, a tap shifted by one row, the
  mask of the wrong layer or pass, a tile-edge row taken from the neighbouring sample, a row group skipped or
  counted twice, a slot skipped, an offset off by one sample, dgrad's dZ staged one row late, the plain
  sigmoid at a saturated logit, the moment normaliser rounded to a float: the largest deviation on the
  entries a mistake touches is at least 10 allowances (a condition on the allowances: one that fails it is
  too wide and has to be derived again);
* the widened-entry rule of the staging's inner bf16 rounding: the reference evaluated in fp32 alone, with
  the staging's multiply-add fused or not, stays inside the widened allowance on every entry of the
  fixtures used."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng

from . import generic_kernel_refs as G
from . import train_kernel_refs as T

POWER = 10.0
N, SEED = 6, 7
Z = torch.zeros((), dtype=torch.float64)


def _ratio(dev, allow):
    dev, allow = dev.abs().reshape(-1), allow.expand(dev.shape).reshape(-1) if allow.shape != dev.shape else allow.reshape(-1)
    r = torch.where(allow > 0, dev / allow.clamp(min=1e-300), torch.where(dev > 0, torch.full_like(dev, float("inf")),
                                                                          torch.zeros_like(dev)))
    return float(r.max())


def _caught(mut, ref, allow):
    assert _ratio(mut - ref, allow) >= POWER


# ------------------------------------------------------------------------------------------ composition
def test_composed_references_match_float64_autograd():
    p = {k: v.double() for k, v in T.params(3).items()}
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(N, T.L, T.CH[0], generator=gen, dtype=torch.float64)
    y = (torch.rand(N, generator=gen) > 0.5).double()
    out = T.step64(p, x, y, SEED, rnd=False)
    q = {k: v.clone().requires_grad_(not k.startswith("batchnorm") or k.endswith(("gamma", "beta"))) for k, v in p.items()}
    logits = R.forward(T.SPEC, q, x, dropout=True, bn_batch_stats=True, update_moving=True, seed=SEED, pass_id=T.PASS,
                       sample_ids=torch.arange(N), return_logits=True, dtype=torch.float64)
    lv = torch.nn.functional.binary_cross_entropy_with_logits(logits.reshape(-1), y, reduction="none")
    lv.mean().backward()
    assert float((out["logits"] - logits.detach().reshape(-1)).abs().max()) <= 1e-9
    assert abs(float(out["loss"]) - lv.sum().item()) <= 1e-9 * lv.sum().item()
    for k, v in q.items():
        ref = v.grad if v.requires_grad else v.detach()
        got = out[k].reshape(ref.shape)
        assert float((got - ref).abs().max()) <= 1e-9 * max(float(ref.abs().max()), 1e-3), k


# ------------------------------------------------------------------------------------------ fixtures
def _layer_inputs(l, n=N, dropout=True, wrong=None):
    """Staged input of block l (A, amb), its kernel / bias, and what it was staged from."""
    p = T.params(3)
    w, b = p[f"conv1d_{l + 1}/kernel"], p[f"conv1d_{l + 1}/bias"]
    if l == 0:
        x = T.bf(torch.randn(n, T.L, T.CH[0], generator=T._gen(1, n)).double())
        return x, None, w, b, None
    mag, drop = T.act_fixture(l - 1, n, SEED, dropout)
    if wrong is not None:   # the mask of another layer id / pass, same shape
        drop = ~rng.keep_mask_torch(rng.stream_key(SEED, *wrong), torch.arange(n), T.L, T.CH[l], T.RATES[l - 1])
    rows = T.table_rows(mag, p[f"batchnorm_{l}/gamma"], p[f"batchnorm_{l}/beta"], n)
    a, amb = T.stage64(mag, drop, rows["s"], rows["t"], T.dsc(l - 1) if dropout else 1.0)
    return a, amb, w, b, (mag, drop, rows)


def _tap_shift(x, w, tap):
    only = torch.zeros_like(w)
    only[tap] = w[tap]
    xs = torch.zeros_like(x)
    xs[:, :-1] = x[:, 1:]
    return G.conv64(x, w) - G.conv64(x, only) + G.conv64(xs, only)


def _no_sample_edges(x, w, b):
    """The conv with every sample's halo rows taken from its neighbours instead of zeros."""
    n, L_, c = x.shape
    return G.conv64(x.reshape(1, n * L_, c), w, b).reshape(n, L_, -1)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("l", range(6))
def test_fwd_allowance_catches_mistakes(l):
    a, amb, w, b, _ = _layer_inputs(l)
    wb = T.bf(w.double())
    ref, allow, nw = T.fwd64(a, w, b, amb=amb)
    print(f"fwd {l}: {nw} of {ref.numel()} entries widened")
    drop = ref.clone()
    drop[-1, -1] = 0
    _caught(drop, ref, allow)                                                     # a row never written
    _caught(torch.relu(_tap_shift(a, wb, T.KS[l] // 2) + b.double()), ref, allow)  # a tap shifted by one row
    _caught(torch.relu(_no_sample_edges(a, wb, b)), ref, allow)                   # edge rows from the neighbour
    _caught(ref.roll(1, 0), ref, allow)                                           # off by one sample
    if l > 0:
        for wrong in ((l, T.PASS), (l - 1, T.PASS + 1)):                          # mask of layer l + 1 / next pass
            a2 = _layer_inputs(l, wrong=wrong)[0]
            _caught(T.fwd64(a2, w, b)[0], ref, allow)
    # moments of the stored tile: one row tile (2 samples) skipped or counted twice; grid 512 and one
    # workgroup over all tiles (the longest chain)
    stored = T.bf(ref)
    for grid in (512, 1):
        m, am = T.fwd_moments(stored, N, grid, l)
        _caught(m - G.moments64(stored[:2]), m, am)
        assert float((am[:, 0])[0]) == 0.0      # the all-zero channel: nothing allowed


@pytest.mark.parametrize("l", [1, 3, 5])
def test_widened_entries_cover_the_fp32_staging(l):
    """The forward reference run in fp32 alone, its staging fma fused (one rounding) or not (two), rounded to
    bf16: inside the widened allowance on every entry."""
    for dropout in (True, False):
        a, amb, w, b, (mag, drop, rows) = _layer_inputs(l, n=5, dropout=dropout)
        ref, allow, nw = T.fwd64(a, w, b, amb=amb)
        assert nw < ref.numel() // 2      # the widening stays the exception
        sc = T.dsc(l - 1) if dropout else 1.0
        s0, t0 = T.f32(rows["s"] * sc).float(), T.f32(rows["t"] * sc).float()
        m32 = mag.float()
        fused = (mag * s0.double() + t0.double()).float()
        unfused = m32 * s0 + t0
        wb = w.bfloat16().float()
        for v in (fused, unfused):
            a32 = torch.where(drop, torch.zeros(()), v.bfloat16().float())
            y32 = torch.relu(R.conv1d_same(a32, wb, b)).bfloat16().double()
            assert _ratio(y32 - ref, allow) <= 1.0


# ------------------------------------------------------------------------------------------ BN rows
def test_bn_row_allowances_catch_mistakes():
    C = T.CH[6]
    p = T.params(3)
    gamma, beta = p["batchnorm_6/gamma"].clone(), p["batchnorm_6/beta"]
    gamma[2] = 1.0
    st = T.bn_edge_slots(C, 1)
    ic = 1.0 / T.BN_COUNT
    r = T.bn_rows64(st, ic, gamma, beta)
    al = T.bn_rows_allow(r, gamma, beta)
    assert abs(float(r["mean"][2]) - 100.0) < 1e-2 and 0.5e-4 < float(r["var"][2]) < 2e-4
    assert float(r["var"][1]) <= 1e-15 and float(r["var"][4]) > 1e6
    skipped = st.clone()
    skipped[5] = 0
    for mut in (T.bn_rows64(skipped, ic, gamma, beta),                      # a slot skipped
                T.bn_rows64(st, 1.0 / (T.BN_COUNT + T.L), gamma, beta)):      # the count off by one sample
        for k in ("mean", "rstd", "s", "t"):
            _caught(mut[k], r[k], al[k])
    # the moment normaliser as a float: the near-constant channel's rstd, s, t are off by far more
    flt = T.bn_rows64(st, float(torch.tensor(ic).float()), gamma, beta)
    for k in ("rstd", "s", "t"):
        assert float((flt[k][2] - r[k][2]).abs() / al[k][2]) >= POWER, k
    bst = torch.randn(T.SLOTS, 2, C, generator=T._gen(2), dtype=torch.float64)
    m, am = T.slot_mean64(bst, ic)
    bs = bst.clone()
    bs[5] = 0
    _caught(T.slot_mean64(bs, ic)[0], m, am)


def test_finalize_allowances_catch_mistakes():
    C = T.CH[6]
    p = T.params(3)
    st = T.bn_edge_slots(C, 1)
    bst = torch.randn(T.SLOTS, 2, C, generator=T._gen(3), dtype=torch.float64)
    hp = torch.randn(T.SLOTS, C + 2, generator=T._gen(4))
    ic = 1.0 / T.BN_COUNT
    mm, mv = p["batchnorm_6/moving_mean"], p["batchnorm_6/moving_variance"]
    ref, al = T.finalize64(st, bst, ic, mm, mv, hp)
    s2, b2, h2 = st.clone(), bst.clone(), hp.clone()
    s2[5], b2[5], h2[5] = 0, 0, 0
    mut, _ = T.finalize64(s2, b2, ic, mm, mv, h2)
    for k in ref:
        _caught(mut[k], ref[k], al[k])
    # (the normaliser as a float moves the near-constant channel's moving variance by a few allowances only:
    # the update weighs the batch variance by 1 - momentum; the table rows are where that defect shows)
    flt, _ = T.finalize64(st, bst, float(torch.tensor(ic).float()), mm, mv, hp)
    print("moving variance, float normaliser:", float((flt["mvar"][2] - ref["mvar"][2]).abs() / al["mvar"][2]))


# ------------------------------------------------------------------------------------------ head
def _head_inputs(n, bias, wrong=None):
    p = T.params(3)
    mag, drop = T.act_fixture(5, n, SEED)
    if wrong is not None:
        drop = ~rng.keep_mask_torch(rng.stream_key(SEED, *wrong), torch.arange(n), T.L, T.CH[6], T.RATES[5])
    rows = T.table_rows(mag, p["batchnorm_6/gamma"], p["batchnorm_6/beta"], n)
    y = (torch.rand(n, generator=T._gen(5, n)) > 0.5).double()
    return mag, drop, rows, p["output_layer/kernel"], bias, y


@pytest.mark.parametrize("bias", [0.25, 30.0, -30.0])
def test_head_allowances_catch_mistakes(bias):
    n = 37
    mag, drop, rows, w, b, y = _head_inputs(n, bias)
    r = T.head64(mag, drop, rows, w, b, y, 1.0 / n, T.dsc(5))
    for mode in ("slots", "atomic", "det"):
        al = T.head_allow(r, n, 1.0 / n, mode)
        m2 = T.head64(mag[:, :-1], drop[:, :-1], rows, w, b, y, 1.0 / n, T.dsc(5))     # a time step dropped
        _caught(m2["logit"] * (T.L - 1) / T.L + b / T.L, r["logit"], al["logit"])
        for wrong in ((4, T.PASS), (5, T.PASS + 1)):                                    # wrong layer id / pass
            d2 = _head_inputs(n, bias, wrong)[1]
            _caught(T.head64(mag, d2, rows, w, b, y, 1.0 / n, T.dsc(5))["logit"], r["logit"], al["logit"])
        _caught(T.head64(mag, drop, rows, w, b, y.roll(1), 1.0 / n, T.dsc(5))["dlog"], r["dlog"], al["dlog"])
        # a sample skipped / counted twice in the sums (the one with the largest gradient: a saturated,
        # correctly labelled sample adds next to nothing)
        i = int(r["dlog"].abs().argmax())
        one = T.head64(mag[i:i + 1], drop[i:i + 1], rows, w, b, y[i:i + 1], 1.0 / n, T.dsc(5))
        for k in ("gw", "gb", "loss", "bst"):
            _caught(r[k] + one[k], r[k], al[k])
    # the plain sigmoid 1 / (1 + exp(-z)) - y in fp32: a probability saturated at 1.0f cancels against its
    # label (at -30 the plain form loses only what a fast exp loses, which a CPU cannot show)
    if bias == 30.0:
        z32 = r["logit"].float()
        plain = ((1.0 / (1.0 + torch.exp(-z32))) - y.float()).double() / n
        sat = y == 1.0
        assert sat.any()
        al = T.head_allow(r, n, 1.0 / n, "slots")
        assert float(((plain - r["dlog"]).abs() / al["dlog"])[sat].max()) >= POWER


# ------------------------------------------------------------------------------------------ dgrad / wgrad
def _bwd_inputs(l, n=N):
    """Block l's R_l, dY_l, table rows and the rows of block l - 1."""
    p = T.params(3)
    mag, drop = T.act_fixture(l, n, SEED)
    rows = T.table_rows(mag, p[f"batchnorm_{l + 1}/gamma"], p[f"batchnorm_{l + 1}/beta"], n)
    dy = T.grad_fixture(l, n, SEED)
    bst = torch.stack([dy.sum((0, 1)), (dy * (mag - rows["mean"]) * rows["rstd"]).sum((0, 1))])
    m = T.f32(bst / (n * T.L))
    return p, mag, drop, rows, dy, m


@pytest.mark.parametrize("l", range(1, 6))
def test_dgrad_allowances_catch_mistakes(l):
    p, mag, drop, rows, dy, m = _bwd_inputs(l)
    dz, a_dz = T.dz64(mag, dy, rows["s"], rows["mean"], rows["rstd"], m[0], m[1])
    a_dz = a_dz + T.UB * dz.abs()
    _caught(dz.roll(1, 0), dz, a_dz)                                            # off by one sample
    _caught(T.dz64(mag, dy, rows["s"], rows["mean"], rows["rstd"], m[0] * 0, m[1])[0], dz, a_dz)  # mean dY lost
    dzs = T.bf(dz)
    w = p[f"conv1d_{l + 1}/kernel"]
    magp, dropp = T.act_fixture(l - 1, N, SEED)
    ref, al = T.dgrad64(dzs, w, ~dropp, T.dsc(l - 1))
    wt = G.flip_t(T.bf(w.double()))
    late = torch.zeros_like(dzs)
    late[:, 1:] = dzs[:, :-1]                                                   # dZ staged one row late
    _caught(T.dgrad64(late, w, ~dropp, T.dsc(l - 1))[0], ref, al)
    gone = ref.clone()
    gone[-1, -1] = 0
    _caught(gone, ref, al)                                                      # a row never written
    sc = T.dsc(l - 1)
    _caught(torch.where(~dropp, _tap_shift(dzs, wt, T.KS[l] // 2) * sc, Z), ref, al)
    _caught(torch.where(~dropp, _no_sample_edges(dzs, wt, None) * sc, Z), ref, al)
    for wrong in ((l, T.PASS), (l - 1, T.PASS + 1)):
        k2 = rng.keep_mask_torch(rng.stream_key(SEED, *wrong), torch.arange(N), T.L, T.CH[l], T.RATES[l - 1])
        _caught(T.dgrad64(dzs, w, k2, sc)[0], ref, al)
    pr = T.table_rows(magp, p[f"batchnorm_{l}/gamma"], p[f"batchnorm_{l}/beta"], N)
    dys = T.bf(ref)
    b, ab = T.bwd_sums64(dys, magp, pr["mean"], pr["rstd"])
    _caught(b + T.bwd_sums64(dys[:2], magp[:2], pr["mean"], pr["rstd"])[0], b, ab)   # a tile counted twice


@pytest.mark.parametrize("l", range(6))
def test_wgrad_allowances_catch_mistakes(l):
    n = 37
    p, mag, drop, rows, dy, m = _bwd_inputs(l, n)
    dz = T.bf(T.dz64(mag, dy, rows["s"], rows["mean"], rows["rstd"], m[0], m[1])[0])
    a, amb = _layer_inputs(l, n)[:2]
    gw, gb, a_gw, a_gb, nw = T.wgrad64(a, dz, l, n, amb=amb)
    print(f"wgrad {l}: {nw} of {gw.numel()} entries widened")
    rgs, rt = T.wg(l, n)["rgs"], T.wg(l, n)["rt"]
    last = 2 * rt * (rgs - 1)                                                    # first sample of the last row group
    g2, b2 = T.wgrad64(a[:last], dz[:last], l, n)[:2]
    _caught(g2, gw, a_gw)                                                        # the last row group dropped
    _caught(b2, gb, a_gb)
    _caught(2 * gw - g2, gw, a_gw)                                               # ... counted twice
    ash = torch.zeros_like(a)
    ash[:, :-1] = a[:, 1:]
    g3 = T.wgrad64(ash, dz, l, n)[0]
    _caught(g3[T.KS[l] // 2], gw[T.KS[l] // 2], a_gw[T.KS[l] // 2])              # a tap shifted by one row
    _caught(T.wgrad64(a, dz.roll(1, 0), l, n)[0], gw, a_gw)                      # off by one sample
    if l > 0:
        a4 = _layer_inputs(l, n, wrong=(l, T.PASS))[0]
        _caught(T.wgrad64(a4, dz, l, n)[0], gw, a_gw)                            # the mask of layer l + 1
