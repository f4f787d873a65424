"""The oracle of the gx3 kernel pins (``tests/gx3_kernel_refs.py``) checked without a GPU: the split bound
derived from the fp16 format, the launcher mirror against the figures each case is named for, the model tier
against float64 truth on every fixture, the exactness conditions of the probes, and -- for every mistake the
GPU file is meant to catch -- a mutation of the model that moves the tier named next to it by >= 10
allowances (bitwise tiers: by at least one entry, their allowance being 0)."""
import math

import pytest
import torch

from . import gx3_kernel_refs as X
from . import generic_kernel_refs as G


# ------------------------------------------------------------------------------------------------ tier 1
def test_prescale_exp_edges():
    assert [X.prescale_exp(v) for v in (0.0, float("inf"), float("nan"), -1.0)] == [14, 14, 14, 14]
    assert X.prescale_exp(1.0) == 13 and X.prescale_exp(0.125) == 16
    assert X.prescale_exp(float(torch.nextafter(torch.tensor(0.125), torch.tensor(0.0)))) == 17
    assert X.prescale_exp(1e-35) == 100 and X.prescale_exp(3e35) == -100
    for v in (3.7e-9, 0.99, 1.0, 517.3, 8191.9, 2.0 ** 20):
        assert 2.0 ** 13 <= v * 2.0 ** X.prescale_exp(v) < 2.0 ** 14


def test_split_residual_bound_from_the_fp16_format():
    """|a - hi - lo| <= max(2^-22 |a|, 2^-25) for every scaled magnitude from the fp16 maximum down to
    below the smallest subnormal, the bound is reached to within a factor 2 in both regimes, and lo is
    subnormal from |a| < 2^-3 down: 2^-16 of a maximum in [2^13, 2^14), not 2^-25 of it."""
    g = torch.Generator().manual_seed(5)
    worst_rel = worst_floor = 0.0
    for e in range(-30, 14):
        a = ((1 + torch.rand(20000, generator=g)) * 2.0 ** e).float()
        hi, lo = X.split(a, 0)
        r = (a.double() - hi.double() - lo.double()).abs()
        bound = torch.maximum(X.SPLIT_REL * a.double().abs(), torch.tensor(X.SPLIT_FLOOR, dtype=torch.float64))
        assert bool((r <= bound).all()), e
        assert bool((lo.double().abs() <= 2.0 ** -11 * a.double().abs() + 2.0 ** -25).all())
        if e >= -3:
            worst_rel = max(worst_rel, float((r / a.double().abs()).max()) / X.SPLIT_REL)
        else:
            assert bool((lo.float().abs() < 2.0 ** -14).all())       # lo subnormal (or zero)
            worst_floor = max(worst_floor, float(r.max()) / X.SPLIT_FLOOR)
    assert 0.5 <= worst_rel <= 1.0 and 0.5 <= worst_floor <= 1.0


# ------------------------------------------------------------------------------------------------ mirror
@pytest.mark.parametrize("case", X.CONV_CASES)
def test_launcher_mirror_reaches_the_named_path(case):
    cin, L, k, cout, n = case
    P = X.conv_path(n, L, cin, cout, k)
    assert (P["path"], P["CT"], P["grid"], P["span"], P["lds"]) == X.CONV_EXPECT[case]
    assert 0 <= P["tap0"] < P["tap1"] <= k and 0 <= P["s0"] < P["s1"] <= P["nstep"]
    assert P["tap1"] - P["tap0"] == min(k, 2 * L - 1)    # the taps that can reach a row of the sample
    assert P["lds"] <= 160 * 1024 - 64 and (not P["halo"] or P["span"] <= 256)
    assert sum(sum(c) for c in P["nc"]) == P["nct"]      # every channel tile on exactly one wave


def test_launcher_mirror_named_properties():
    P = {c: X.conv_path(c[4], c[1], c[0], c[3], c[2]) for c in X.CONV_CASES}
    assert P[(64, 60, 5, 128, 9)]["nc"] == [[4, 4]]
    assert P[(32, 60, 7, 96, 9)]["nc"] == [[3, 3]]
    assert P[(32, 15, 9, 36, 9)]["nc"] == [[3, 0]] and P[(32, 15, 9, 36, 9)]["last_tile"] == 4
    assert P[(32, 15, 9, 36, 9)]["lds"] > 64 * 1024 > P[(224, 60, 7, 132, 9)]["lds"]
    assert P[(224, 60, 7, 132, 9)]["nc"] == [[4, 4], [1, 0]] and P[(224, 60, 7, 132, 9)]["last_tile"] == 4
    assert X.conv_path(9, 8, 32, 48, 9)["span"] == 0 and 128 + 16 * 8 + 8 == 264       # one past the limit
    assert (P[(96, 3, 9, 20, 9)]["tap0"], P[(96, 3, 9, 20, 9)]["tap1"]) == (2, 7)
    assert (P[(256, 1, 7, 12, 9)]["tap0"], P[(256, 1, 7, 12, 9)]["tap1"]) == (3, 4)
    assert (P[(256, 1, 7, 12, 9)]["s0"], P[(256, 1, 7, 12, 9)]["s1"]) == (24, 32)
    # the dgrad of (36, 15, 3, 100) at L = 1 would start inside a k-step; here: s0 of a short sequence
    Q = X.conv_path(9, 1, 36, 100, 3)
    assert Q["tap0"] == 1 and Q["s0"] == 1 and 36 % 32 != 0
    assert P[(4, 60, 7, 256, 9)]["nc"] == [[4, 4], [4, 4]]


@pytest.mark.parametrize("case", X.WGRAD_CASES)
def test_wgrad_mirror(case):
    cin, k, cout, n, L, slices = case
    R = n * (L + k - 1)
    groups, rpg = X.wgrad_path(R, cin, cout, k, slices * k * cin * cout)
    assert (groups, rpg) == X.WGRAD_EXPECT[case]
    assert rpg % 64 == 0 and (groups - 1) * rpg < R <= groups * rpg
    assert X.wgrad_path(R, cin, cout, k, k * cin * cout - 1) == (0, 0)     # one float short: rejected


def test_wgrad_cases_cover_what_they_name():
    ks = {c[1] for c in X.WGRAD_CASES}
    assert ks == {1, 3, 5, 7, 9, 11, 15}
    assert {c[0] for c in X.WGRAD_CASES} >= {1, 3, 36, 100, 224}
    assert {c[2] for c in X.WGRAD_CASES} >= {12, 48, 100, 256}
    Rs = [c[3] * (c[4] + c[1] - 1) for c in X.WGRAD_CASES]
    assert 1 in Rs and any(1 < r < 64 for r in Rs) and 576 in Rs


# ------------------------------------------------------------------------------------------------ model vs truth
def _model_vs_truth(M, truth, a2, name):
    r = X.ratio(M - truth, a2)
    print(f"[ratio] model vs float64 {name}: {r:.4f}")
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("case", X.CONV_CASES)
def test_conv_model_matches_truth(case):
    R = X.conv_refs(case)
    _model_vs_truth(R["fwd"]["y"], R["fwd_truth"], R["fwd_a2"], "forward")
    if "dgr" in R:
        _model_vs_truth(R["dgr"]["y"], R["dgr_truth"], R["dgr_a2"], "dgrad")
    # the precision claim: the truth allowance is far below the accumulation allowance and ~1e-6 of the terms
    assert float((R["fwd_a2"] / R["fwd"]["ab"]).max()) < 4 * 2.0 ** -22 * 1.5


@pytest.mark.parametrize("case", X.WGRAD_CASES)
def test_wgrad_model_matches_truth(case):
    R = X.wgrad_refs(case)
    _model_vs_truth(R["model"]["gw"], R["truth"], R["a2"], "wgrad")
    _model_vs_truth(R["model_up"]["gw"], R["truth"], R["a2_up"], "wgrad, amax words 2^10 above")
    # the widened floor is what the larger words cost: the plain allowance no longer holds them
    assert bool((R["a2_up"] > R["a2"]).all())


def _mixed(case):
    cin, L, k, cout, n = case
    x, w, b, dz = X.mixed_fixture(*case)
    F = X.conv_model(x, w, b, relu=True)
    D = X.conv_model(dz, X.flip_t(w)) if cin % 4 == 0 else None
    return x, w, b, dz, F, D


@pytest.mark.parametrize("case", X.MIXED_CASES)
def test_mixed_magnitude_model_matches_truth(case):
    """Every entry, the 2^-18 window's included, within the allowance with its floor; without the floor the
    small window's entries are NOT held (the floor is what the mixed tile costs, the documented limit)."""
    cin, L, k, cout, n = case
    x, w, b, dz, F, D = _mixed(case)
    assert [t[2:4] for t in X.tiles(x, L)] == [(0, 8), (8, 8)]
    assert F["sb"][0] != F["sb"][-1]
    a2 = X.truth_allow(x, w, F["sb"], F["sw"])
    _model_vs_truth(F["y"], X.conv_truth(x, w, b, True), a2, "mixed forward")
    if D is not None:
        wf = X.flip_t(w)
        t = X.conv_truth(dz, wf)
        _model_vs_truth(D["y"], t, X.truth_allow(dz, wf, D["sb"], D["sw"]), "mixed dgrad")
        rel_only = X.SLACK * 3 * X.SPLIT_REL * X.conv_abs64(dz, wf).reshape(t.shape)
        assert X.ratio(D["y"] - t, rel_only) > 10.0
    xp, dzp = X.padded(x, k, True), X.padded(dz, k, False)
    R = dzp.shape[0]
    W = X.wgrad_model(xp, dzp, R, k, X.amax32(x), X.amax32(dz))
    _model_vs_truth(W["gw"], X.wgrad64(xp, dzp, R, k)[0], X.wgrad_truth_allow(xp, dzp, R, k, W["sx"], W["sd"]), "mixed wgrad")


def test_neighbour_dependence_of_the_model():
    """Beyond 2^+-5 a window's result depends on its tile neighbours: the 2^-18 window next to a 2^12 one
    against the same window alone, relative to the window's largest output -- the figure of the docs."""
    case = X.MIXED_CASES[0]
    cin, L, k, cout, n = case
    x, w, b, dz, F, D = _mixed(case)
    alone = X.conv_model(dz[5:6], X.flip_t(w))["y"]       # the 2^-18 window of dz (rotated by 2)
    assert float(dz[5].abs().max()) < 2.0 ** (-18 + X.MIXED_DZ_SHIFT + 3)
    tile = D["y"][5 * L: 6 * L]
    rel = float((tile - alone).abs().max() / alone.abs().max())
    print(f"[figure] neighbour dependence of the 2^-18 window (model): {rel:.3e}")
    assert 2.0 ** -16 < rel < 2.0 ** -6


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", X.CONV_CASES)
def test_probe_fixtures_are_exact(case):
    cin, L, k, cout, n = case
    dgrad = cin % 4 == 0
    x, dz = X.probe_acts(n, L, cin, 0), X.probe_acts(n, L, cout, 1)
    exps = sorted({t[4] for t in X.tiles(x, L)} | {t[4] for t in X.tiles(dz, L)})
    for v in (x, dz):
        assert X.split_is_scale_free(v, exps)
        hi, lo = X.split(v, exps[0])
        assert bool((hi != 0).all()) and bool((lo != 0).all())
    nets = X.probe_nets(k, cin, cout, dgrad)
    cover_f = torch.zeros(k, cin, dtype=torch.bool)
    cover_d = torch.zeros(k, cout, dtype=torch.bool)
    b = X.probe_bias(cout)
    for w in nets:
        wh, wl = X.split(w, X.prescale_exp(X.amax32(w)))
        assert bool(((wl != 0) & (wh != 0)).any())
        cover_f |= (w != 0).any(2)
        cover_d |= (w != 0).any(1)
        M = X.conv_model(x, w, b, relu=False)
        assert X.is_exact(M["y"], M["ab"])
        assert torch.equal(M["y"], X.conv_truth(x, w, b) - X.conv64(*_lolo(x, w, M)).reshape(M["y"].shape))
        if dgrad:
            D = X.conv_model(dz, X.flip_t(w))
            assert X.is_exact(D["y"], D["ab"])
    assert bool(cover_f.all()) and (not dgrad or bool(cover_d.all()))
    # wgrad probe
    p = (k - 1) // 2
    xp = X.padded(x, k, True)
    R = n * (L + 2 * p)
    dzs = X.probe_sparse_dz(R, cout, 0)
    assert bool((dzs != 0).any(1).all())
    W = X.wgrad_model(xp, dzs, R, k, X.amax32(xp), X.amax32(dzs))
    assert X.is_exact(W["gw"], W["ab"])


def _lolo(x, w, M):
    """The dropped lo lo term (exact in float64 for the probes): truth - model must equal it."""
    _, xl = X.halves64(x, int(M["sb"][0]))
    _, wl = X.halves64(w, M["sw"])
    return xl, wl


# ------------------------------------------------------------------------------------------------ mutations
def _moved(mut, ref, allow, what):
    r = X.ratio(mut - ref, allow)
    print(f"[moved] {what}: {r:.3g} allowances")
    return r


def test_mutations_dropped_terms_move_the_exact_tier():
    """A dropped lo hi or hi lo MFMA: caught by the exact probes (bitwise; any differing entry), forward,
    dgrad and wgrad.  (At K ~ 1500 the accumulation allowance is wider than the dropped term.)"""
    cin, L, k, cout, n = 32, 15, 9, 36, 9
    x, dz = X.probe_acts(n, L, cin, 0), X.probe_acts(n, L, cout, 1)
    w = X.probe_nets(k, cin, cout, True)[0]
    for v, ww in ((x, w), (dz, X.flip_t(w))):
        ref = X.conv_model(v, ww)["y"]
        for d in ("lo_hi", "hi_lo"):
            assert int((X.conv_model(v, ww, drop=(d,))["y"] != ref).sum()) > ref.numel() // 2
    xp = X.padded(x, k, True)
    R = n * (L + 8)
    dzs = X.probe_sparse_dz(R, cout, 0)
    ref = X.wgrad_model(xp, dzs, R, k, 16.0, 2.0)["gw"]
    for d in ("lo_hi", "hi_lo"):
        assert int((X.wgrad_model(xp, dzs, R, k, 16.0, 2.0, drop=(d,))["gw"] != ref).sum()) > ref.numel() // 4


def test_mutations_wrong_exponent_move_the_mixed_tier():
    """Sample n0's exponent for the tile, the neighbouring tile's exponent, amax of the wrong operand:
    invisible at one magnitude per launch (a power-of-two prescale commutes with the fp16 rounding), caught
    by the mixed-magnitude tier per entry (hi overflows, or a window is flushed)."""
    case = X.MIXED_CASES[0]
    cin, L, k, cout, n = case
    x, w, b, dz, F, D = _mixed(case)
    a = X.acc_allow(F["ab"], k * cin) + X.truth_allow(x, w, F["sb"], F["sw"])
    T = X.tiles(x, L)
    n0_only = [X.prescale_exp(X.amax32(x[t[2]: t[2] + 1])) for t in T]
    assert n0_only != [t[4] for t in T]
    assert _moved(X.conv_model(x, w, b, True, exps=n0_only)["y"], F["y"], a, "sample n0's exponent for the tile") >= 10
    swapped = [T[1][4], T[0][4]]
    assert _moved(X.conv_model(x, w, b, True, exps=swapped)["y"], F["y"], a, "the neighbouring tile's exponent") >= 10
    # one magnitude per launch: the same mutations change nothing
    x1, w1, b1, _ = X.conv_fixture(*case)
    x1[5:] *= 0.25        # tiles of different exponents, yet one magnitude: no half leaves the normal range
    T1 = X.tiles(x1, L)
    assert T1[0][4] != T1[1][4]
    plain = X.conv_model(x1, w1, b1, True)
    wrong = X.conv_model(x1, w1, b1, True, exps=[T1[1][4] - 1, T1[0][4] - 1])["y"]
    assert _moved(wrong, plain["y"], X.acc_allow(plain["ab"], k * cin), "a wrong exponent at one magnitude") < 0.01
    xp, dzp = X.padded(x, k, True), X.padded(dz, k, False)
    R = dzp.shape[0]
    ax, ad = X.amax32(x), X.amax32(dz)
    W = X.wgrad_model(xp, dzp, R, k, ax, ad)
    aw = X.wgrad_acc_allow(W["ab"], R, 1) + X.wgrad_truth_allow(xp, dzp, R, k, W["sx"], W["sd"])
    assert _moved(X.wgrad_model(xp, dzp, R, k, ad, ax)["gw"], W["gw"], aw, "amax of the wrong operand") >= 10


def test_mutations_geometry_move_the_random_tier():
    """A tap shifted at an edge row, a neighbour's row for a pad row, tap0 off by one at L < k, swapped channel
    tiles, a dropped wgrad row group: caught by the random cases per entry."""
    case = (96, 3, 9, 20, 9)
    cin, L, k, cout, n = case
    R = X.conv_refs(case)
    x, w, b = R["x"], R["w"], R["b"]
    ref, a = R["fwd"]["y"], R["fwd_a1"] + R["fwd_a2"]
    # tap shifted at the first row of every sample
    xs = torch.zeros_like(x)
    xs[:, :-1] = x[:, 1:]
    mut = ref.clone().view(n, L, cout)
    mut[:, 0] = X.conv_model(xs, w, b, True)["y"].view(n, L, cout)[:, 0]
    assert _moved(mut.reshape(ref.shape), ref, a, "a tap shifted at an edge row") >= 10
    # the neighbour's rows where the pad rows should be
    mut = torch.relu(X.conv64(x.reshape(1, n * L, cin), w, b)).reshape(ref.shape)
    assert _moved(mut, ref, a, "a neighbour's row for a pad row") >= 10
    # tap0 off by one: the first tap in range never issued
    P = X.conv_path(n, L, cin, cout, k)
    w0 = w.clone()
    w0[P["tap0"]] = 0
    assert _moved(X.conv_model(x, w0, b, True)["y"], ref, a, "tap0 off by one at L < k") >= 10
    # swapped channel tiles
    case = (32, 15, 9, 36, 9)
    R = X.conv_refs(case)
    ref, a = R["fwd"]["y"], R["fwd_a1"] + R["fwd_a2"]
    mut = ref.clone()
    mut[:, 0:16], mut[:, 16:32] = ref[:, 16:32], ref[:, 0:16]
    assert _moved(mut, ref, a, "swapped channel tiles") >= 10
    # wgrad: the last row group dropped
    wc = X.WGRAD_CASES[2]
    Rw = X.wgrad_refs(wc)
    groups, rpg = X.wgrad_path(Rw["R"], wc[0], wc[2], wc[1], wc[5] * wc[0] * wc[1] * wc[2])
    mut = X.wgrad_model(Rw["xp"], Rw["dzp"], Rw["R"], wc[1], Rw["ax"], Rw["ad"], rows=slice(0, (groups - 1) * rpg))["gw"]
    assert _moved(mut, Rw["model"]["gw"], Rw["a1"] + Rw["a2"], "a row group dropped") >= 10


def test_mutations_moment_slots_move_the_moment_tier():
    """A skipped or doubled moment slot (the deterministic index without its wave row): caught by the moment
    sums and by the per-slot comparison."""
    case = (64, 60, 5, 128, 9)
    R = X.conv_refs(case)
    u, e = R["fwd"]["y"], R["fwd_a1"]
    rows = u.shape[0]
    slots = X.slot_moments(u)
    assert slots.shape[0] == 2 * X.conv_path(9, 60, 64, 128, 5)["grid"][0]
    assert torch.allclose(slots.sum(0), G.moments64(u), rtol=1e-12, atol=0)
    allow = G.moments_allow(u, e, G.conv_chain(rows, True))
    skipped = slots.sum(0) - slots[3]
    doubled = slots.sum(0) + slots[2]
    no_wr = slots[1::2].sum(0)      # blockIdx.x * 2 for both wave rows: the second overwrites the first
    for what, mut in (("a skipped moment slot", skipped), ("a doubled moment slot", doubled),
                      ("the slot index without its wave row", no_wr)):
        assert _moved(mut, G.moments64(u), allow, what) >= 10


# ------------------------------------------------------------------------------------------------ fixtures
def test_neighbour_fixture_condition():
    """The halves of every window are the same at every exponent its tile can take, in the full launch and
    launched from window 3 on: the condition under which the GPU test demands bitwise equal rows."""
    for case in X.MIXED_CASES:
        cin, L, k, cout, n = case
        x, w, b = X.neighbour_fixture(*case)
        assert max(X.NEIGHBOUR_EXPS) - min(X.NEIGHBOUR_EXPS) <= 10
        every = set()
        for s in range(n):
            # the exponents of the tiles that hold rows of window s, in the full launch and from window 3 on
            exps = {t[4] for t in X.tiles(x, L) if t[2] <= s <= t[3]}
            if s >= 3:
                exps |= {t[4] for t in X.tiles(x[3:], L) if t[2] <= s - 3 <= t[3]}
            assert X.split_is_scale_free(x[s], sorted(exps))
            every |= exps
        assert len(every) > 1
        exps = sorted(every)
        assert bool((X.split(x, exps[-1])[1] != 0).any())
        full = X.conv_model(x, w, b, True)["y"]
        sub = X.conv_model(x[3:], w, b, True)["y"]
        assert torch.equal(full[3 * L:], sub)


def test_pack_reference_order():
    """``frag_order`` against the element-by-element statement of the fragment layout."""
    w = torch.arange(5 * 3 * 20, dtype=torch.float32).reshape(5 * 3, 20)
    f = X.frag_order(w)
    assert f.shape == (1, 2, 64, 8)
    for ct, lane, j in ((0, 0, 0), (0, 17, 3), (1, 3, 7), (1, 35, 6), (1, 63, 7), (0, 31, 6)):
        kk, co = 8 * (lane // 16) + j, 16 * ct + lane % 16
        assert float(f[0, ct, lane, j]) == (float(w[kk, co]) if kk < 15 and co < 20 else 0.0)
    ws = X.pack_weights()
    assert X.amax32(ws[3]) == 0 and X.amax32(ws[4]) == 0.125 and X.amax32(ws[5]) < 0.125
    sws = [X.pack_ref(wt, False)[1] for wt in ws]
    assert sws[3:] == [14, 16, 17, 100, -100]
    assert all(math.ldexp(1.0, -s) > 0 for s in sws)
