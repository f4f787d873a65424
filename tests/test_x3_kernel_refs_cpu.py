"""The float64 oracle of the x3 engine's kernels (``tests/x3_kernel_refs.py``) checked where no GPU is needed:

* composed into a whole forward, ``l1_ref`` -> ``aff_ref`` -> ``layer_ref`` x 5 -> ``head_ref`` with the masks of
  ``ops/rng.py`` reproduce ``models/reference.py:forward(..., dtype=float64)`` to 1e-5 in the logit, for the
  running-statistics MC Dropout (per-sample prescale from ``sample_prescale_ref``) and for the batch-moment one
  (per-group prescale from ``aff_ref``'s moments, as ``x3_aff`` gscale folds it).  What is left is the 22 bits
  of the fp16 split and the fp32 rounding of the staged activations: measured 1.7e-8 (running, logits up to 0.54) and 1.6e-7
  (batch, logits up to 0.20) on 6 windows;
* every allowance and bound is at least ``POWER`` = 10 times below the effect of a real mistake, on the fixtures
  of ``tests/test_x3_kernels_gpu.py``: another slot's exponent (in staging, in the epilogue, in both), the
  neighbouring window's ``smax``, the mask of the wrong layer or pass, a tap shifted by a row, a halo row taken
  from the neighbouring window, a moment slot skipped, a ``float`` normaliser, ``repeat`` applied once, groups
  updated in reverse order, the head reading group 0's affine or dense weights, 1/64 for 1/60;
* the fixtures keep every prescale bound away from a power of two (``near_pow2``): the share of cases excluded
  for an fp32 bound that could round across one is zero."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng, x3

from . import generic_kernel_refs as G
from . import x3_kernel_refs as X
from .test_generic_kernel_refs_cpu import _tap_shift

POWER = 10.0
L = X.L


# ================================================================================================ composition
def _params():
    p = R.synthetic_params(SPEC, 9)
    gen = torch.Generator().manual_seed(4)
    for k in p:
        if k.endswith("/bias"):
            p[k] = (torch.randn(p[k].shape, generator=gen) * 0.1).float()
    return p


def _bn(p, l, stats=None, inv_count=1.0):
    names = ("gamma", "beta", "moving_mean", "moving_variance")
    gamma, beta, mm, mv = (p[f"batchnorm_{l + 1}/{n}"].float()[None] for n in names)
    return dict(stats=stats, gamma=gamma, beta=beta, mmean=mm, mvar=mv, inv_count=inv_count, C=gamma.shape[1], groups=1,
                p_gstride=0)


def _compose(p, x, seed, pass_id, batch):
    """One pass of MC Dropout over windows ``x`` from the per-kernel references -> logits (n,)."""
    n = x.shape[0]
    ids = torch.arange(n)
    rates = [b.dropout for b in SPEC.blocks]
    dsc = [float(np.float32(1.0 / (1.0 - r))) for r in rates]
    r = X.l1_ref(x, p["conv1d_1/kernel"][None], p["conv1d_1/bias"][None])[0][0]

    def affine(l, r):
        """Block l + 1's affine for the consumer: (aff (2, C) fp32, per-sample exponents or None, accumulator factor)."""
        if batch:
            st = torch.zeros(1, X.SLOTS, 2, r.shape[2], dtype=torch.float64)
            st[0, 5] = G.moments64(r)
            F = _bn(p, l, st, 1.0 / (n * L))
            A = X.aff_ref(F, "batch_gscale", dsc[l])
            sa = int(X.prescale_exp(X.gscale_bound(A["s"], A["t"], A["q"]))[0])
            return torch.stack([A["s"][0], A["t"][0]]).mul(2.0 ** sa).float(), None, 2.0 ** -sa
        A = X.aff_ref(_bn(p, l), "moving_amax", dsc[l])
        aff = torch.stack([A["s"][0], A["t"][0]]).float()
        sa = X.sample_prescale_ref(X.amax_of(aff[None])[0], r.float().amax((1, 2)))[0]
        return aff, sa, 1.0

    for l in range(1, 6):
        cin, cout, k = x3.CH[l], x3.CH[l + 1], x3.KS[l]
        aff, sa, gs = affine(l - 1, r)
        keep = rng.keep_mask_torch(rng.stream_key(seed, l - 1, pass_id), ids, L, cin, rates[l - 1])
        fr, sc = x3.pack_conv(p[f"conv1d_{l + 1}/kernel"])
        r = X.layer_ref(r.float(), aff, keep, fr, sc * gs, p[f"conv1d_{l + 1}/bias"], k, cin, cout, sa)
    if batch:   # block 6 feeds the fp32 head: its affine carries no prescale
        st = torch.zeros(1, X.SLOTS, 2, r.shape[2], dtype=torch.float64)
        st[0, 11] = G.moments64(r)
        A = X.aff_ref(_bn(p, 5, st, 1.0 / (n * L)), "batch", dsc[5])
        aff = torch.stack([A["s"][0], A["t"][0]]).float()
    else:
        aff = affine(5, r)[0]
    keep = rng.keep_mask_torch(rng.stream_key(seed, 5, pass_id), ids, L, x3.CH[6], rates[5])
    s1, s0 = X.block6_sums(r[None], keep[None])
    F = dict(sums=torch.stack([s1[0], s0[0].double()], 1), aff=aff[None], dw=p["output_layer/kernel"].reshape(1, -1),
             db=p["output_layer/bias"].reshape(1), n_win=n, groups=1, aff_gstride=0, p_gstride=0)
    return X.head_ref(F)[0]


@pytest.mark.parametrize("batch", [False, True])
def test_composed_references_match_float64_forward(batch):
    p = _params()
    n, seed, pass_id = 6, 11, 3
    x = torch.randn(n, L, 4, generator=torch.Generator().manual_seed(5)).float()
    got = _compose(p, x, seed, pass_id, batch)
    p64 = {k: v.double() for k, v in p.items()}
    want = R.forward(SPEC, p64, x.double(), dropout=True, bn_batch_stats=batch, seed=seed, pass_id=pass_id,
                     sample_ids=torch.arange(n), return_logits=True, dtype=torch.float64).reshape(-1)
    err = float((got - want).abs().max())
    print(f"composed {'batch' if batch else 'running'} chain: max |logit error| {err:.3e} (logits up to {float(want.abs().max()):.2f})")
    assert err <= 1e-5


# ================================================================================================ block 1
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("n_win", X.L1_NWIN)
def test_l1_allowances_catch_mistakes(n_win, groups):
    x, w, b = X.l1_fixture(n_win, groups)
    want, allow = X.l1_ref(x, w, b)
    tap = X.ratio(X.l1_ref(x, w, b, conv=lambda x, wg: _tap_shift(x, wg, 2))[0] - want, allow)
    assert tap >= POWER, tap
    if n_win >= 2:   # the halo rows of a window read from its neighbours: one long sequence
        chain = lambda x, wg: G.conv64(x.reshape(1, -1, 4), wg).reshape(n_win, L, -1)
        halo = X.ratio(X.l1_ref(x, w, b, conv=chain)[0] - want, allow)
        assert halo >= POWER, halo
    # moments: the slot of one workgroup (8 windows) left out of the sum
    out = want.float()
    msum = X.stored_moments(out)
    skipped = X.stored_moments(out[:, 8:]) if n_win > 8 else torch.zeros_like(msum)
    assert X.ratio(skipped - msum, X.l1_moment_allow(msum)) >= POWER
    # smax of the neighbouring window differs in its bits wherever the two windows' maxima do
    if n_win >= 2:
        bits = X.window_max_bits(out)
        assert (bits != bits.roll(1, 1)).any()


# ================================================================================================ BN affine
@pytest.mark.parametrize("layout", X.AFF_LAYOUTS)
@pytest.mark.parametrize("C", X.AFF_C)
def test_aff_allowances_catch_mistakes(C, layout):
    groups, pgs = layout
    F = X.aff_fixture(C, groups, pgs is None)
    ref = X.aff_ref(F, "batch", X.DSC)
    # a float normaliser: the near-constant channel (group 0, channel 0) loses its variance
    mut = X.aff_ref(F, "batch", X.DSC, inv_count=float(np.float32(F["inv_count"])))
    assert X.ratio(mut["s"] - ref["s"], ref["a_s"]) >= POWER
    # a slot skipped
    used = int((F["stats"][0].abs().sum((1, 2)) > 0).nonzero()[0])
    F2 = dict(F, stats=F["stats"].clone())
    F2["stats"][:, used] = 0.0
    mut = X.aff_ref(F2, "batch", X.DSC)
    assert X.ratio(mut["s"] - ref["s"], ref["a_s"]) >= POWER and X.ratio(mut["t"] - ref["t"], ref["a_t"]) >= POWER
    # repeat applied once
    ref5 = X.aff_ref(F, "update5", 1.0)
    mut = X.aff_ref(F, "update5", 1.0, once=True)
    assert X.ratio(mut["mm"] - ref5["mm"], ref5["a_mm"]) >= POWER and X.ratio(mut["mv"] - ref5["mv"], ref5["a_mv"]) >= POWER
    # groups updated last to first: matters where they update the same moving averages
    if groups > 1 and not F["p_gstride"]:
        for mode in ("update1", "update5"):
            ref_u = X.aff_ref(F, mode, 1.0)
            mut = X.aff_ref(F, mode, 1.0, reverse=True)
            assert X.ratio(mut["mm"] - ref_u["mm"], ref_u["a_mm"]) >= POWER, mode
            # (C = 1: the one channel's variances are 1e-4, 0 and 0 in the three groups, nothing to reorder)
            assert C == 1 or X.ratio(mut["mv"] - ref_u["mv"], ref_u["a_mv"]) >= POWER, mode


def test_aff_fixture_bounds_are_off_the_powers_of_two():
    """The excluded share is zero: no gscale bound of any fixture is within 2^-18 of a power of two, so the fp32
    bound and the float64 one have the same exponent.  (The GPU file asserts it again on the kernel's own s, t.)"""
    fixtures = [(X.aff_fixture(C, g, p is None), 1.0 if i % 2 else X.DSC)
                for i, C in enumerate(X.AFF_C) for g, p in X.AFF_LAYOUTS]
    fixtures += [(X.aff_fixture(C, 3, True, kind), X.DSC) for C in (1, 300) for kind in X.AFF_EXTREMES]
    exps = set()
    for F, _ in fixtures:
        for dsc in (1.0, X.DSC):
            for mode in ("batch_gscale", "running_gscale"):
                A = X.aff_ref(F, mode, dsc)
                bnd = X.gscale_bound(A["s"], A["t"], A["q"])
                assert not X.near_pow2(bnd).any(), (F["C"], F["groups"], mode, bnd.tolist())
                exps |= set(X.prescale_exp(bnd).tolist())
    assert {-100, 14, 100} <= exps and len(exps) > 4   # both clamps, the zero bound, and ordinary exponents


# ================================================================================================ layers, PS
def _shift_rows(h, fr, wscale, k, cin, cout):
    """The split product with tap 1 reading the row after the one it should."""
    y = x3.emulate_conv(h, fr, wscale, k, cin, cout)
    w = x3.unpack_conv(fr, wscale, k, cin, cout)
    only = torch.zeros_like(w)
    only[1] = w[1]
    hs = torch.zeros_like(h)
    hs[:, :-1] = h[:, 1:]
    return y - G.conv64(h, only) + G.conv64(hs, only)


@pytest.mark.parametrize("l,n_win,variant", [c for c in X.PS_CASES if c[1] == 11])
def test_layer_ps_bound_catches_mistakes(l, n_win, variant):
    c = X.ps_case(l, n_win, variant)
    for g in range(X.GROUPS):
        assert not X.near_pow2(X.ps_exponents(c, g)[1]).any()
    want = X.layer_ps_ref(c)
    bound = POWER * X.REL_BOUND
    j = X.window_exps(n_win)

    def rel(**kw):
        return X.per_sample_rel(X.layer_ps_ref(c, **kw), want)

    # another slot's exponent: a sample between neighbours of another scale is off by their power of two
    assert rel(stage=X.neighbour).max() >= bound and rel(epi=X.neighbour).max() >= bound
    # ... in both: the value survives but the split is taken at the wrong scale.  Every 2^12 window overflows fp16.
    # The affine shift t dominates the bound of the 2^-18 windows here (their exponent is that of t alone), so
    # this fixture cannot expose them: the equivariance fixture (t = 0) below does
    both = rel(stage=X.neighbour, epi=X.neighbour)
    assert all(both[:, w].min() >= bound for w in range(n_win) if j[w] == 12)
    # the neighbouring window's smax: the same, through the bound
    sm = c["smax_in"].view(-1, n_win)
    idx = (torch.arange(n_win) ^ 1).clamp_max(n_win - 1)
    assert rel(smax=sm[:, idx].reshape(-1)).max() >= bound
    # the mask of the wrong layer or pass (where this call hashes one)
    if c["rate_in"] and not c["sign_in"]:
        assert rel(layer_shift=1).min() >= bound and rel(pass_shift=1).min() >= bound
    # a tap shifted by a row (the staged rows of a 2^-18 window are the constant shift t: nothing to see there
    # without a mask)
    assert rel(conv=_shift_rows)[:, j != -18].min() >= bound


@pytest.mark.parametrize("l,n_win,variant", [c for c in X.PS_CASES if c[1] == 11])
def test_scale_equivariance_catches_a_shared_exponent(l, n_win, variant):
    """Check 2 of the GPU file on the emulation: B = 2^j A holds for the reference to the last bit of its fp32
    store, and with the neighbouring slot's exponent in staging and epilogue alike it breaks on the 2^12 and
    2^-18 windows by far more than 10 REL_BOUND."""
    j = X.window_exps(n_win)
    base = X.ps_case(l, n_win, variant, exps=torch.zeros(n_win, dtype=torch.int64), zero_shift=True, zero_bias=True)
    scaled = X.scale_windows(base, j)
    f = torch.pow(2.0, j.double())[None, :, None, None]
    a, b = X.layer_ps_ref(base), X.layer_ps_ref(scaled)
    assert torch.equal(b.float(), (a * f).float())
    kw = dict(stage=X.neighbour, epi=X.neighbour)
    am, bm = X.layer_ps_ref(base, **kw), X.layer_ps_ref(scaled, **kw)
    assert not torch.equal(X.f32_bits(bm.float()), X.f32_bits((am * f).float()))
    rel = X.per_sample_rel(bm, am * f)
    for w in range(n_win):
        if j[w] in (12, -18) and (w ^ 1) < n_win:
            assert rel[:, w].min() >= POWER * X.REL_BOUND, (w, rel[:, w].tolist())


# ================================================================================================ head
@pytest.mark.parametrize("bias", X.HEAD_BIASES)
@pytest.mark.parametrize("shape", [s for s in X.HEAD_SHAPES if s[1] > 1])
def test_head_allowances_catch_mistakes(shape, bias):
    F = X.head_fixture(*shape, True, True, bias)
    z, a_z, p, a_p = X.head_ref(F)
    for kw in (dict(inv=1.0 / 64), dict(aff_group0=True), dict(dense_group0=True)):
        zm, _, pm, _ = X.head_ref(F, **kw)
        assert X.ratio(zm - z, a_z) >= POWER, kw
        if abs(bias) < 1:   # a saturated probability hides everything: the logits carry those cases
            assert X.ratio(pm - p, a_p) >= POWER, kw
    assert float(a_p.min()) >= 2.0 ** -126
