"""The oracle of the batch-moment x3 layer kernels (``tests/x3_layer_refs.py``) checked where no GPU is needed:

* the model (fp16 halves, hi hi + lo hi + hi lo) lies within its derived allowance of plain float64 truth on every
  fixture of ``tests/test_x3_layer_kernels_gpu.py``;
* every probe satisfies its exactness conditions (each fma exact, staged = hi + lo, every entry's terms on one grid
  and below 2^24 units) and has the stated share of elements with lo != 0;
* every ``n_win`` has the tile geometry it is named for, from ``tiles_per_group`` / ``tile_geo`` as the committed
  layer table of ``csrc/x3_geo.h`` gives them;
* composed with the ``l1`` / ``aff`` / ``head`` references the model reproduces
  ``models/reference.py:forward(dtype=float64)`` under batch moments;
* each mistake a kernel could make moves its tier by at least ``POWER`` = 10 allowances, or a probe by at least one
  grid unit (``test_*_catch*``)."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng, x3

from . import generic_kernel_refs as G
from . import x3_kernel_refs as X
from . import x3_layer_refs as T

POWER = 10.0
L = T.L


# ================================================================================================ geometry
def test_layer_table_is_the_one_the_fixtures_assume():
    tab = T.layer_table()
    assert sorted(tab) == T.LAYERS
    for l, (cin, cout, k, S, dense) in tab.items():
        assert (cin, cout, k) == (x3.CH[l], x3.CH[l + 1], x3.KS[l])
        assert S == T.TILE_S[l] and dense == (l < 5)
    assert [l for l in T.LAYERS if T.tile_rows(l) == 128] == [2, 4]
    assert [l for l in T.LAYERS if T.tile_rows(l) == 256] == [1, 3, 5]


@pytest.mark.parametrize("l", T.LAYERS)
def test_window_counts_have_the_geometry_they_are_named_for(l):
    S, rows, pad = T.TILE_S[l], T.tile_rows(l), (x3.KS[l] - 1) // 2
    ns = T.nwin_cases(l)
    # below and across a slot tile of 4 samples (of 2: at, below and across)
    assert ns[:4] == [1, 2, 3, 5]
    assert [T.tiles_per_group(False, n, 4) for n in (1, 2, 3, 5)] == [1, 1, 1, 2]
    assert T.tiles_per_group(False, 5, S) == -(-5 // S) > 1 and T.tiles_per_group(False, 1, S) == 1

    def last(n):
        tpg = T.tiles_per_group(True, n, S)
        return tpg, T.tile_geo(True, S, tpg - 1, tpg, n)

    if rows == 128:
        assert ns[4:] == [15, 32]
        tpg, geo = last(15)
        assert 15 * L == 900 and tpg == 8 and geo["rows_left"] == 4
        assert x3.KS[4] == 9 and (9 - 1) // 2 == 4          # ... which equals PAD at k = 9 (layer 4)
        tpg, geo = last(32)
        assert tpg == 15 and geo["rows_left"] == 128
    else:
        assert ns[4:] == [47, 64]
        tpg, geo = last(47)
        assert 47 * L == 2820 and tpg == 12 and geo["rows_left"] == 4
        tpg, geo = last(64)
        assert tpg == 15 and geo["rows_left"] == 256
    # a dense tile starts inside a window and a window boundary falls inside a tile
    tpg = T.tiles_per_group(True, 5, S)
    offs = [T.tile_geo(True, S, t, tpg, 5)["off"] for t in range(tpg)]
    assert any(offs) and pad >= 1
    # grids: 1 walks every tile and both group changes; the largest leaves every workgroup at most one tile
    for dense in (False, True):
        total = T.GROUPS * T.tiles_per_group(dense, T.PROBE_NWIN, S)
        assert 3 < total <= T.GRIDS[-1]
        assert T.tiles_per_slot(dense, l, T.PROBE_NWIN, T.GROUPS, 1) == T.tiles_per_group(dense, T.PROBE_NWIN, S)
        assert T.tiles_per_slot(dense, l, T.PROBE_NWIN, T.GROUPS, T.GRIDS[-1]) == 1


# ================================================================================================ model vs truth
def _check_truth(r, tag):
    ratio = X.ratio(r["M"]["y"] - r["T"], r["a2"])
    print(f"{tag}: model against truth, |err| / allowance {ratio:.3f}")
    assert ratio <= 1.0
    # the two allowances: the accumulation allowance is the wider one at these K
    assert (r["a2"] > 0).all() and (r["M"]["a1"] > 0).all()


@pytest.mark.parametrize("l,n_win,variant", T.tier1_cases())
def test_model_within_truth_allowance(l, n_win, variant):
    r = T.tier1_refs(l, n_win, variant)
    c = r["c"]
    _check_truth(r, f"layer {l} n_win {n_win} {variant}")
    # the fixture is what it says: three exponents, negative and zero scales, small entries, a finite split
    assert c["gscale"].tolist() == [2.0 ** -e for e in T.GROUP_EXPS[:len(c["gscale"])]]
    s = c["aff"][:, 0]
    assert (s < 0).any() and (s == 0).any() and (s > 0).any()
    assert len(set(c["scs"])) == len(c["scs"])                       # every member its own wscale
    lo, hi = T.staged_range(c)
    assert hi < 2.0 ** 14 and lo < hi * 2.0 ** -11
    assert any((h < 0).any() for h in r["M"]["h"])                   # R >= 0 under a negative scale
    y = r["M"]["y"]
    small = y[..., torch.arange(c["cout"]) % 16 == 7]
    assert 0 < float(small.max()) < float(y.max()) * 2.0 ** -8


@pytest.mark.parametrize("l", T.LAYERS)
def test_equivariance_fixture_and_aff_chain_within_truth_allowance(l):
    c = T.case(l, 3, "hash", equivariant=True)
    for d in (c, T.rescale_groups(c, T.EQUI_J)):
        lo, hi = T.staged_range(d)
        assert 2.0 ** -3 <= lo and hi < 2.0 ** 14, (lo, hi)
        M = T.model(d)
        Tr, a2 = T.truth(d, M)
        _check_truth(dict(M=M, T=Tr, a2=a2), f"layer {l} equivariance fixture")
    # the model itself is equivariant to the last bit of its fp32 store ...
    a, b = T.model(c), T.model(T.rescale_groups(c, T.EQUI_J))
    assert T.bits_differ(a["y"].float(), b["y"].float()) == 0
    # ... and a kernel reading group 0's gscale for every group is not
    m = T.model(T.rescale_groups(c, T.EQUI_J), gscale_of=lambda g: 0)
    assert T.bits_differ(a["y"].float(), m["y"].float()) > 0
    # x3_aff's own chain: three different exponents, no bound on a power of two
    c = T.aff_chain_case(l, 3)
    aff, sa, bnd = T.aff_chain_expected(c)
    print(f"layer {l}: x3_aff exponents {sa.tolist()} of bounds {bnd.tolist()}")
    assert len(set(sa.tolist())) == 3 and not X.near_pow2(bnd).any()
    c["aff"], c["gscale"] = aff.float(), torch.pow(2.0, -sa.double()).float()
    lo, hi = T.staged_range(c)
    assert hi < 2.0 ** 14
    M = T.model(c)
    Tr, a2 = T.truth(c, M)
    _check_truth(dict(M=M, T=Tr, a2=a2), f"layer {l} x3_aff chain")


# ================================================================================================ probes
@pytest.mark.parametrize("l,n_win,variant", T.probe_cases())
def test_probes_are_exact(l, n_win, variant):
    r = T.probe_refs("probe", l, n_win, variant)
    c, M = r["c"], r["M"]
    assert T.probe_exact(c, M)
    share = T.lo_share(c, M)
    # 7 of 8 channels have a non-zero scale and every value of theirs a lo; a mask keeps 70 % of them
    want = 0.85 if variant == "plain" else 0.55
    print(f"layer {l} n_win {n_win} {variant}: share of lo != 0 {share:.3f}")
    assert share >= want
    # every window is non-zero on its first and last PAD rows, and every k-row of every tap carries a weight
    pad = (c["k"] - 1) // 2
    for h in M["h"]:
        assert (h[:, :pad].abs().amax((1, 2)) > 0).all() and (h[:, -pad:].abs().amax((1, 2)) > 0).all()
    assert all((w.abs().amax(2) > 0).all() for w in c["w"])
    assert (c["bias"] > 0).any() and (c["bias"] < 0).any() and torch.equal(c["bias"], c["bias"].round())
    assert float(M["y"].max()) > 0


@pytest.mark.parametrize("variant", T.PS_VARIANTS)
@pytest.mark.parametrize("l", T.LAYERS)
def test_ps_probes_are_exact(l, variant):
    r = T.probe_refs("ps", l, T.PROBE_NWIN, variant)
    c, M = r["c"], r["M"]
    assert T.probe_exact(c, M)
    sa, bnd = T.probe_sa(c)
    assert not X.near_pow2(bnd).any()
    assert sorted(set((10 - sa[0]).tolist())) == sorted(T.PROBE_PS_EXPS)     # five magnitudes in one launch
    assert len(set(sa[0][:T.TILE_S[l]].tolist())) == T.TILE_S[l]            # ... and different ones inside a tile


@pytest.mark.parametrize("variant", T.MOMENT_VARIANTS)
@pytest.mark.parametrize("l", T.LAYERS)
def test_moment_probes_are_exact(l, variant):
    r = T.probe_refs("moment", l, T.PROBE_NWIN, variant)
    c, M = r["c"], r["M"]
    assert T.probe_exact(c, M) and T.lo_share(c, M) == 0.0
    y = M["y"]
    assert torch.equal(y, y.round()) and 0 < float(y.max()) <= 15
    assert float((y * y).sum((1, 2)).max()) < 2.0 ** 24                      # a group's sums, so every tile's


@pytest.mark.parametrize("variant,ps", T.S1_CASES)
def test_block6_s1_probe_is_exact_and_sees_a_dropped_half(variant, ps):
    """Block 6's only output is S1 / S0 and the moments: the probe keeps S1 itself exact with lo != 0 on both sides,
    and a dropped half moves S1 -- the quantity the GPU test compares bit for bit -- by whole units, on every row or
    at a single entry."""
    r = T.s1_probe_refs(variant, ps)
    c, M = r["c"], r["M"]
    assert T.probe_exact(c, M)
    assert T.lo_share(c, M) >= (0.85 if variant == "plain" else 0.55)
    assert all((w != w.half().float()).any() for w in c["w"])                # a lo in the weights too
    assert all(int((w != 0).sum(0).reshape(-1).max()) <= 2 for w in (w.reshape(-1, c["cout"]) for w in c["w"]))
    keep = T.out_keep(c)
    assert keep.any() and ((~keep).any() or variant == "plain")
    u = T.s1_units(c, M["y"])
    assert torch.equal(u, u.round()) and 0 < float(u.max()) < 2.0 ** 24 and (u > 0).float().mean() > 0.5
    s1 = T.block6_sums(M["y"], keep)[0]
    assert torch.equal(s1.float().double(), s1)                               # ... and fits an fp32
    for d in ("lo_hi", "hi_lo"):
        m = T.probe_model(c, drop=(d,))
        moved = (T.s1_units(c, m["y"]) - u).abs()
        # one entry alone: the kept entries that move at all move S1 by a whole unit or more
        e = ((m["y"] - M["y"]).abs() * keep / c["unit"])
        print(f"S1 probe {variant} ps {ps}: dropped {d} moves {int((moved > 0).sum())} of {moved.numel()} sums by up to "
              f"{float(moved.max()):.0f} units; {int((e > 0).sum())} entries by {float(e[e > 0].min()):.0f} or more")
        assert float(moved.max()) >= 1.0 and (moved > 0).float().mean() > 0.5
        assert (e > 0).float().mean() > 0.25 and float(e[e > 0].min()) >= 1.0


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


def _layer(r, aff, gs, keep, w, b):
    k, cin, cout = w.shape
    fr, sc = x3.pack_conv(w)
    _, ah, al = T.stage(r.float(), aff, keep)
    y, _ = T.split_product(ah, al, *T.frag_halves(fr, k, cin, cout))
    return (y * (sc * gs) + b.double()).clamp_min(0.0)


def test_composed_references_match_float64_forward():
    """l1_ref -> (aff_ref with gscale -> this file's model) x 5 -> aff_ref -> head_ref, one MC-Dropout pass under
    batch moments."""
    p = _params()
    n, seed, pass_id = 6, 11, 3
    x = torch.randn(n, L, 4, generator=torch.Generator().manual_seed(5)).float()
    ids = torch.arange(n)
    rates = [b.dropout for b in SPEC.blocks]
    dsc = [float(np.float32(1.0 / (1.0 - r))) for r in rates]
    r = X.l1_ref(x, p["conv1d_1/kernel"][None], p["conv1d_1/bias"][None])[0][0]

    def bn(l, r, mode):
        st = torch.zeros(1, X.SLOTS, 2, r.shape[2], dtype=torch.float64)
        st[0, 5] = G.moments64(r)
        return X.aff_ref(_bn(p, l, st, 1.0 / (n * L)), mode, dsc[l])

    for l in range(1, 6):
        A = bn(l - 1, r, "batch_gscale")
        sa = int(X.prescale_exp(X.gscale_bound(A["s"], A["t"], A["q"]))[0])
        aff = torch.stack([A["s"][0], A["t"][0]]).mul(2.0 ** sa).float()
        keep = rng.keep_mask_torch(rng.stream_key(seed, l - 1, pass_id), ids, L, x3.CH[l], rates[l - 1])
        r = _layer(r, aff, 2.0 ** -sa, keep, p[f"conv1d_{l + 1}/kernel"], p[f"conv1d_{l + 1}/bias"])
    A = bn(5, r, "batch")
    keep = rng.keep_mask_torch(rng.stream_key(seed, 5, pass_id), ids, L, x3.CH[6], rates[5])
    s1, s0 = T.block6_sums(r[None], keep[None])
    F = dict(sums=torch.stack([s1[0], s0[0].double()], 1), aff=torch.stack([A["s"][0], A["t"][0]]).float()[None],
             dw=p["output_layer/kernel"].reshape(1, -1), db=p["output_layer/bias"].reshape(1), n_win=n, groups=1,
             aff_gstride=0, p_gstride=0)
    got = X.head_ref(F)[0]
    p64 = {k: v.double() for k, v in p.items()}
    want = R.forward(SPEC, p64, x.double(), dropout=True, bn_batch_stats=True, seed=seed, pass_id=pass_id,
                     sample_ids=ids, return_logits=True, dtype=torch.float64).reshape(-1)
    err = float((got - want).abs().max())
    print(f"composed batch-moment chain: max |logit error| {err:.3e} (logits up to {float(want.abs().max()):.2f})")
    assert err <= 1e-5


# ================================================================================================ mutations, tier 1
@pytest.mark.parametrize("l", T.LAYERS)
def test_tier1_allowances_catch_mistakes(l):
    n = T.PROBE_NWIN
    r = T.tier1_refs(l, n, "hash")
    c, M = r["c"], r["M"]
    allow = M["a1"] + r["a2"]

    def moved(**mut):
        """Blocks 2..5: the stored entries; block 6, which stores none: S1 under its own allowance."""
        m = T.model(c, **mut)
        if l < 5:
            return X.ratio(m["y"] - M["y"], allow)
        keep = T.out_keep(c)
        return X.ratio(T.block6_sums(m["y"], keep)[0] - T.block6_sums(M["y"], keep)[0], T.s1_allow(M["y"], M["a1"], keep))

    figs = dict(gscale0=moved(gscale_of=lambda g: 0), aff0=moved(aff_of=lambda g: 0), wscale0=moved(wscale_of=lambda g: 0),
                mask_layer=moved(mask=dict(layer_shift=1)), mask_pass=moved(mask=dict(same_pass=True)),
                mask_window_offset=moved(mask=dict(win_off=0)), mask_halves=moved(mask=dict(swap=True)))
    print(f"layer {l}: allowances moved by " + ", ".join(f"{k} {v:.3g}" for k, v in figs.items()))
    assert min(figs.values()) >= POWER, figs
    # the output side: the mask this call draws (sign bits, S0) under the same four mistakes is another mask
    s = T.tier1_refs(l, n, "sign")["c"] if l < 5 else c
    if s["sign_out"] or l == 5:
        keep = T.out_keep(s)
        assert (~keep).any() and keep.any()
        for mut in (dict(layer_shift=-1), dict(same_pass=True), dict(win_off=0), dict(swap=True)):
            other = T.out_keep(s, **mut)
            assert (other != keep).any()
            assert float((other.sum(2) - keep.sum(2))[1:].abs().max()) >= 1   # S0 of the groups past the first, in steps
    # moments: one row past the group's end counted (its accumulator is 0, so it holds relu(bias))
    y = M["y"]
    msum = T.moments(y)
    rb = torch.stack([c["bias"][T.gw(c, g)].double().clamp_min(0.0) for g in range(T.GROUPS)])
    extra = torch.cat([rb, rb * rb], 1)
    for dense in ([False, True] if l < 5 else [False]):
        assert T.past_end_rows(dense, l, n) >= 1
        al = T.moment_allow(msum, dense, l, n, T.GRID)
        fig = X.ratio(extra, al if l < 5 else al + T.model_moment_allow(y, M["a1"]))
        print(f"layer {l} {'dense' if dense else 'slot'}: a counted row past the end moves the moments by {fig:.3g} allowances")
        # block 6's moments are held to the model's sums, the entries' allowances carried: one row is far inside
        # that (0.05 allowances).  Its tier for this mistake is the exact small-output probe (test_probes_catch_mistakes)
        assert fig >= POWER or l == 5, fig
    # block 6: S1 of the neighbouring sample
    if l == 5:
        keep = T.out_keep(c)
        s1 = T.block6_sums(y, keep)[0]
        fig = X.ratio(torch.roll(s1, 1, 1) - s1, T.s1_allow(y, M["a1"], keep))
        print(f"layer {l}: S1 of the neighbour moves the allowance by {fig:.3g}")
        assert fig >= POWER


# ================================================================================================ mutations, probes
@pytest.mark.parametrize("l", T.LAYERS)
def test_probes_catch_mistakes(l):
    r = T.probe_refs("probe", l, T.PROBE_NWIN, "plain")
    c, M = r["c"], r["M"]

    if l == 5:      # block 6 stores no entries: its probe for the halves is the one whose S1 is exact
        r = T.s1_probe_refs("plain", False)
        c, M = r["c"], r["M"]

    def units(**mut):
        """Largest move in grid units and the stored values that change: entries, or block 6's S1."""
        m = T.probe_model(c, **mut)
        if l < 5:
            return float(((m["core"] - M["core"]).abs() / c["unit"]).max()), T.bits_differ(m["y"].float(), M["y"].float())
        a, b = T.block6_sums(m["y"], T.out_keep(c))[0], T.block6_sums(M["y"], T.out_keep(c))[0]
        return float((T.s1_units(c, m["y"]) - T.s1_units(c, M["y"])).abs().max()), T.bits_differ(a.float(), b.float())

    figs = dict(lo_hi=units(drop=("lo_hi",)), hi_lo=units(drop=("hi_lo",)), tap_shift=units(mode="tap_shift"),
                neighbour=units(mode="neighbour"), past_end=units(mode="past_end"))
    print(f"layer {l}: probe entries moved (grid units, stored entries) {figs}")
    for k, (u, nbits) in figs.items():
        assert u >= 1.0 and nbits > 0, (k, u, nbits)
    # the group mistakes on the probe's three exponents
    for mut in (dict(gscale_of=lambda g: 0),) + ((dict(wscale_of=lambda g: 0),) if l < 5 else ()):   # (one wscale at l = 5)
        u, nbits = units(**mut)
        assert u >= 1.0 and nbits > 0
    # exact moments, S1 and S0: a counted row past the end, a dropped step counted, the neighbour's S1
    r = T.probe_refs("moment", l, T.PROBE_NWIN, "hash")
    c, M = r["c"], r["M"]
    rb = torch.stack([c["bias"][T.gw(c, g)].double().clamp_min(0.0) for g in range(T.GROUPS)])
    assert (rb.amax(1) >= 1).all()                      # a counted row moves a sum by a whole unit (outputs are integers)
    if l == 5:
        keep = T.out_keep(c)
        s1, s0 = T.block6_sums(M["y"], keep)
        first = (~keep).cumsum(2) == 1                  # each (sample, channel)'s first dropped step, counted as kept
        moved = ((keep | (first & ~keep)).sum(2) - s0).abs()
        assert float(moved.max()) >= 1 and (moved >= 1).float().mean() > 0.9
        assert float((torch.roll(s1, 1, 1) - s1).abs().max()) >= 1     # the neighbour's S1, in units (integers)
