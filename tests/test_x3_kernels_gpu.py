"""Every kernel of the fp32-faithful layer-wise engine (``csrc/x3_layers.hip``) launched alone and held to the
float64 references of ``tests/x3_kernel_refs.py``: ``x3_l1``, ``x3_aff`` (its six modes), ``x3_head`` (its four
stride combinations) and the per-sample-prescale (``PS = true``) variants of ``x3_layer``.  The allowances are
derived there; ``tests/test_x3_kernel_refs_cpu.py`` shows what they catch.  Output buffers sit between
``SENTINEL`` guards: the guards stay untouched and every output element is written.

``x3_layer`` PS: stored values are compared per sample, max |got - want| over the sample / max |want| of the
sample, under the rowdesc file's ``REL_BOUND`` (measured on the same k-loop, twice its largest figure);
the scale-equivariance and slice checks are bitwise.  Each test prints its figure before it asserts."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, rng, x3

from . import generic_kernel_refs as G
from . import x3_kernel_refs as X

pytestmark = pytest.mark.gpu

SENTINEL = X.RD.SENTINEL
GUARD = X.RD.GUARD
ISENT = 0x5A5A5A5A        # sentinel of the int32 smax buffers
GROUPS, GRID, SEED, PASS_BASE, WIN_OFF = X.GROUPS, X.GRID, X.SEED, X.PASS_BASE, X.WIN_OFF


def _dev():
    return torch.device("cuda")


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    """(buffer, the n-element view between two guards of GUARD elements)."""
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=_dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=SENTINEL):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all())


# ================================================================================================ x3_l1
def _run_l1(x, w, b, groups, stats, smax):
    o, dev = _ext.ops(), _dev()
    n = x.shape[0]
    buf, out = _guarded(groups * n * 60 * 128)
    st = torch.zeros(groups * X.SLOTS * 2 * 128, dtype=torch.float64, device=dev) if stats else None
    sbuf, sm = _guarded(groups * n, torch.int32, ISENT)
    o.x3_l1(x.to(dev), w.to(dev).contiguous(), b.to(dev).contiguous(), out, st, n, groups, sm if smax else None)
    torch.cuda.synchronize()
    assert _guards_intact(buf, out.numel()), "a store outside the output"
    assert _guards_intact(sbuf, sm.numel(), ISENT), "a store outside smax"
    return (out.cpu().view(groups, n, 60, 128), None if st is None else st.cpu().view(groups, X.SLOTS, 2, 128), sm.cpu().view(groups, n))


def _check_l1(n_win, groups, stats, smax, all_zero=False):
    x, w, b = X.l1_fixture(n_win, groups, all_zero)
    out, st, sm = _run_l1(x, w, b, groups, stats, smax)
    assert not (out == SENTINEL).any(), "rows left unwritten"
    want, allow = X.l1_ref(x, w, b)
    r = X.ratio(out.double() - want, allow)
    tag = f"x3_l1 n_win {n_win} groups {groups} stats {stats} smax {smax}"
    print(f"{tag}: stored values, |err| / allowance {r:.3f}")
    rm = 0.0
    if stats:
        msum = X.stored_moments(out)
        rm = X.ratio(st.sum(1) - msum, X.l1_moment_allow(msum))
        print(f"{tag}: moments, |err| / allowance {rm:.3f}")
        # a group's workgroups (8 windows each) spread over the 16 slots
        assert int((st.abs().sum((2, 3)) > 0).sum(1).max()) <= min(X.SLOTS, -(-n_win // 8))
    if smax:
        assert torch.equal(sm, X.window_max_bits(out)), f"{tag}: smax"
    else:
        assert (sm == ISENT).all()
    if n_win >= 2 or all_zero:      # the zero window under the all-negative bias of the last group
        assert (out[-1, 0] == 0).all() and (not smax or sm[-1, 0] == 0)
    assert r <= 1.0
    assert rm <= 1.0


@pytest.mark.parametrize("smax", [False, True])
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("n_win", X.L1_NWIN)
def test_l1(n_win, groups, stats, smax):
    _ext.require()
    _check_l1(n_win, groups, stats, smax)


def test_l1_single_zero_window():
    _ext.require()
    _check_l1(1, 1, True, True, all_zero=True)


# ================================================================================================ x3_aff
def _run_aff(F, mode, dsc):
    o, dev = _ext.ops(), _dev()
    M = X.aff_mode(mode)
    C, groups = F["C"], F["groups"]
    abuf, aff = _guarded(groups * 2 * C)
    mbuf, am = _guarded(groups * 2)
    gbuf, gs = _guarded(groups)
    mm, mv = F["mmean"].to(dev).contiguous(), F["mvar"].to(dev).contiguous()
    o.x3_aff(F["stats"].to(dev).reshape(-1) if M["stats"] else None, F["gamma"].to(dev).contiguous(),
             F["beta"].to(dev).contiguous(), mm, mv, aff, C, groups, F["p_gstride"], M["update"], M["repeat"],
             F["inv_count"], G.EPS, G.MOMENTUM, dsc, am if M["amax"] else None, gs if M["gscale"] else None, M["running"])
    torch.cuda.synchronize()
    assert _guards_intact(abuf, aff.numel()) and _guards_intact(mbuf, am.numel()) and _guards_intact(gbuf, gs.numel())
    assert not (aff == SENTINEL).any(), "affine entries left unwritten"
    return aff.cpu().view(groups, 2, C), am.cpu().view(groups, 2), gs.cpu(), mm.cpu(), mv.cpu()


def _check_aff(F, mode, dsc, tag):
    M = X.aff_mode(mode)
    aff, am, gs, mm, mv = _run_aff(F, mode, dsc)
    R = X.aff_ref(F, mode, dsc)
    un = aff.double()
    if M["gscale"]:
        e = torch.frexp(gs.double())
        assert (e[0] == 0.5).all(), f"{tag}: gscale is not a power of two: {gs.tolist()}"
        un = un * gs.double()[:, None, None]       # an exact product
        bnd = X.gscale_bound(un[:, 0], un[:, 1], R["q"])
        assert not X.near_pow2(bnd).any(), f"{tag}: a fixture bound on a power of two"
        assert torch.equal(e[1].long() - 1, -X.prescale_exp(bnd)), f"{tag}: exponents {(e[1] - 1).tolist()} bounds {bnd.tolist()}"
    else:
        assert (gs == SENTINEL).all()
    rs, rt = X.ratio(un[:, 0] - R["s"], R["a_s"]), X.ratio(un[:, 1] - R["t"], R["a_t"])
    rmm, rmv = X.ratio(mm.double() - R["mm"], R["a_mm"]), X.ratio(mv.double() - R["mv"], R["a_mv"])
    print(f"{tag}: |err| / allowance scale {rs:.3f} shift {rt:.3f} moving mean {rmm:.3f} variance {rmv:.3f}")
    if M["amax"]:
        assert torch.equal(X.f32_bits(am), X.f32_bits(X.amax_of(aff))), f"{tag}: amax"
    else:
        assert (am == SENTINEL).all()
    if not M["update"]:
        assert torch.equal(mm, F["mmean"]) and torch.equal(mv, F["mvar"]), f"{tag}: moving statistics changed"
    assert max(rs, rt) <= 1.0
    assert max(rmm, rmv) <= 1.0


@pytest.mark.parametrize("mode", X.AFF_MODES)
@pytest.mark.parametrize("layout", X.AFF_LAYOUTS)
@pytest.mark.parametrize("C", X.AFF_C)
def test_aff(C, layout, mode):
    _ext.require()
    groups, pgs = layout
    F = X.aff_fixture(C, groups, pgs is None)
    i = X.AFF_C.index(C) + X.AFF_LAYOUTS.index(layout) + X.AFF_MODES.index(mode)
    dsc = X.DSC if i % 2 else 1.0     # every mode, layout and C meets both
    _check_aff(F, mode, dsc, f"x3_aff C {C} groups {groups} p_gstride {F['p_gstride']} {mode} dsc {dsc:.3f}")


@pytest.mark.parametrize("mode", ["batch_gscale", "running_gscale"])
@pytest.mark.parametrize("kind", X.AFF_EXTREMES)
@pytest.mark.parametrize("C", [1, 300])
def test_aff_extreme_bounds(C, kind, mode):
    """A bound of 0 (gscale 2^-14) and bounds of about 1e-36 / 1e35 (the +-100 clamps)."""
    _ext.require()
    F = X.aff_fixture(C, 3, True, kind)
    _check_aff(F, mode, X.DSC, f"x3_aff C {C} {kind} {mode}")
    gs = _run_aff(F, mode, X.DSC)[2].double()
    want = {"zero": 2.0 ** -14, "tiny": 2.0 ** -100, "huge": 2.0 ** 100}[kind]
    assert (gs == want).all(), gs.tolist()


# ================================================================================================ x3_head
def _run_head(F, logits):
    o, dev = _ext.ops(), _dev()
    n = F["n_win"] * F["groups"]
    buf, out = _guarded(n)
    o.x3_head(F["sums"].to(dev).reshape(-1), F["aff"].to(dev).reshape(-1), F["aff_gstride"], F["dw"].to(dev).reshape(-1),
              F["db"].to(dev), F["p_gstride"], out, F["n_win"], F["groups"], logits)
    torch.cuda.synchronize()
    assert _guards_intact(buf, n), "a store outside the output"
    assert not (out == SENTINEL).any(), "samples left unwritten"
    return out.cpu().double()


@pytest.mark.parametrize("bias", X.HEAD_BIASES)
@pytest.mark.parametrize("per_dense", [False, True])
@pytest.mark.parametrize("per_aff", [False, True])
@pytest.mark.parametrize("shape", X.HEAD_SHAPES)
def test_head(shape, per_aff, per_dense, bias):
    _ext.require()
    n_win, groups = shape
    F = X.head_fixture(n_win, groups, per_aff, per_dense, bias)
    z, a_z, p, a_p = X.head_ref(F)
    rz = X.ratio(_run_head(F, True) - z, a_z)
    rp = X.ratio(_run_head(F, False) - p, a_p)
    print(f"x3_head n_win {n_win} groups {groups} aff_gstride {F['aff_gstride']} p_gstride {F['p_gstride']} bias {bias}: "
          f"|err| / allowance logit {rz:.3f} probability {rp:.3f}")
    assert rz <= 1.0
    assert rp <= 1.0


# ================================================================================================ x3_layer, PS
def _run_ps(c, win_off=WIN_OFF, track=True):
    """One PS launch: dict(out, mom, smax) on the CPU; guards and coverage asserted here."""
    o, dev = _ext.ops(), _dev()
    f32 = dict(dtype=torch.float32, device=dev)
    l, n_win, cout = c["l"], c["n_win"], c["cout"]
    n_out = GROUPS * n_win * (2 * cout if l == 5 else 60 * cout)
    buf, out = _guarded(n_out)
    st = torch.zeros(GROUPS * X.SLOTS * 2 * cout, dtype=torch.float64, device=dev)
    sbuf, smo = _guarded(GROUPS * n_win, torch.int32, ISENT)
    track = track and l < 5
    if track:
        smo.zero_()
    o.x3_layer(l, c["r_in"].to(**f32).contiguous(), out, torch.stack(c["frs"]).to(dev).contiguous(),
               c["frs"][0].numel() // 8 if c["per_group"] else 0, c["bias"].to(**f32).contiguous(),
               torch.tensor(c["scs"], **f32), cout if c["per_group"] else 0, c["aff"].reshape(-1).to(**f32).contiguous(),
               0 if c["shared"] else 2 * c["cin"], st, n_win, GROUPS, c["shared"],
               rng.dropout_threshold(c["rate_in"]) if c["rate_in"] else 0,
               rng.dropout_threshold(c["rate_out"]) if c["rate_out"] else 0, SEED, PASS_BASE, win_off, GRID,
               c["smax_in"].to(dev), c["amax"].reshape(-1).to(**f32).contiguous(), smo if track else None, None,
               c["sign_in"], c["sign_out"], False)
    torch.cuda.synchronize()
    assert _guards_intact(buf, n_out), "a store outside the output"
    assert _guards_intact(sbuf, smo.numel(), ISENT), "a store outside smax_out"
    assert not (out == SENTINEL).any(), "rows left unwritten"
    if not track:
        assert (smo == ISENT).all()
    shape = (GROUPS, n_win, 2, cout) if l == 5 else (GROUPS, n_win, 60, cout)
    return dict(out=out.cpu().view(shape), mom=st.view(GROUPS, X.SLOTS, 2 * cout).sum(1).cpu(),
                smax=smo.cpu().view(GROUPS, n_win))


def _out_keep(c):
    if c["rate_out"]:
        return torch.stack([X.ps_keep(c, g, "out") for g in range(GROUPS)])
    return torch.ones(GROUPS, c["n_win"], 60, c["cout"], dtype=torch.bool)


def _check_against_ref(c, res, tag):
    """Check 1 (and 3): stored values per sample, sign bits, moments, smax_out of one launch against the emulation.
    Returns the largest per-sample figure."""
    l, n_win, cout = c["l"], c["n_win"], c["cout"]
    want = X.layer_ps_ref(c)
    for g in range(GROUPS):
        assert not X.near_pow2(X.ps_exponents(c, g)[1]).any(), f"{tag}: a fixture bound on a power of two"
    out, mom = res["out"], res["mom"]
    assert torch.isfinite(out).all()
    if l < 5:
        if c["sign_out"]:
            keep = _out_keep(c)
            assert torch.equal(torch.signbit(out), ~keep), f"{tag}: {(torch.signbit(out) == keep).sum().item()} sign bits differ"
        else:
            assert not torch.signbit(out).any()
        rel = X.per_sample_rel(out.abs(), want)
        msum = X.stored_moments(out).flatten(1)
        merr = ((mom - msum).abs() / msum.clamp_min(1e-300)).max().item()
        print(f"{tag}: stored values, max per-sample relative error {rel.max().item():.3e}; moments {merr:.3e}")
        # 3. the per-sample maxima: bitwise the max over the sample's stored |out|
        assert torch.equal(res["smax"], X.window_max_bits(out)), f"{tag}: smax_out"
        assert merr <= X.MOMENT_RTOL
    else:
        keep = _out_keep(c)
        s1, s0 = X.block6_sums(want, keep)
        assert torch.equal(out[:, :, 1], s0), f"{tag}: S0"
        rel = X.per_sample_rel(out[:, :, 0][:, :, None], s1[:, :, None])
        msum = torch.cat([want.sum((1, 2)), (want * want).sum((1, 2))], 1)
        merr = (mom - msum).abs() / msum.clamp_min(1e-300)
        peak = torch.cat([want.amax((1, 2)), want.amax((1, 2)) ** 2], 1)
        mtol = X.MOMENT_RTOL + 2 * X.REL_BOUND * peak * n_win * 60 / msum.clamp_min(1e-300)
        print(f"{tag}: S1, max per-sample relative error {rel.max().item():.3e}; moments {merr.max().item():.3e}")
        assert (merr <= mtol).all()
    assert rel.max().item() <= X.REL_BOUND, f"{tag}: per-sample figures {rel.tolist()}"
    return rel.max().item()


@pytest.mark.parametrize("l,n_win,variant", X.PS_CASES)
def test_layer_ps_mixed_scales(l, n_win, variant):
    """Checks 1 and 3: window i scaled by 2^(0, 12, -18, 5, -7)[i % 5], every sample held to the float64 emulation
    on its own scale; sign bits, moments and the per-sample maxima as stored.  Also run without ``smax_out``: the
    stored values are bitwise the same and nothing is tracked."""
    _ext.require()
    c = X.ps_case(l, n_win, variant)
    tag = f"x3_layer PS layer {l} n_win {n_win} {variant}"
    res = _run_ps(c)
    _check_against_ref(c, res, tag)
    if l < 5:
        plain = _run_ps(c, track=False)
        assert torch.equal(X.f32_bits(plain["out"]), X.f32_bits(res["out"])), f"{tag}: tracking changed the output"


@pytest.mark.parametrize("l,n_win,variant", X.PS_CASES)
def test_layer_ps_scale_equivariance(l, n_win, variant):
    """Check 2, bitwise: with bias 0 and affine shift 0 a window times 2^j moves its exponent by exactly j, so the
    staged halves are the same and the output is 2^j times the base launch's, sign bits and maxima included."""
    _ext.require()
    base = X.ps_case(l, n_win, variant, exps=torch.zeros(n_win, dtype=torch.int64), zero_shift=True, zero_bias=True)
    j = X.window_exps(n_win)
    a, b = _run_ps(base), _run_ps(X.scale_windows(base, j))
    f = torch.pow(2.0, j.double()).float()[None, :, None, None]
    tag = f"x3_layer PS layer {l} n_win {n_win} {variant}"
    if l < 5:
        ok = X.f32_bits(b["out"]) == X.f32_bits(a["out"] * f)
        print(f"{tag}: equivariance, {int((~ok).sum())} of {ok.numel()} entries differ")
        assert ok.all(), f"{tag}: windows {sorted(set((~ok).nonzero()[:, 1].tolist()))} are not 2^j times the base"
        assert torch.equal(b["smax"], X.f32_bits(X.bits_f32(a["smax"]) * f[..., 0, 0])), f"{tag}: smax_out"
        assert (a["out"].abs().amax((2, 3)) > 0).all()
    else:
        ok = X.f32_bits(b["out"][:, :, 0]) == X.f32_bits(a["out"][:, :, 0] * f[..., 0])
        print(f"{tag}: equivariance, {int((~ok).sum())} of {ok.numel()} sums differ")
        assert ok.all()
        assert torch.equal(b["out"][:, :, 1], a["out"][:, :, 1]), f"{tag}: S0"


@pytest.mark.parametrize("l,n_win,variant", [c for c in X.PS_CASES if c[1] == 11])
def test_layer_ps_slice_invariance(l, n_win, variant):
    """Check 4, bitwise: windows [3:] launched alone (window_offset + 3, sliced smax_in) reproduce their rows of
    the full launch; every window changes its slot and its tile neighbours."""
    _ext.require()
    a = 3
    c = X.ps_case(l, n_win, variant)
    full, part = _run_ps(c), _run_ps(X.slice_case(c, a), win_off=WIN_OFF + a)
    ok = X.f32_bits(part["out"]) == X.f32_bits(full["out"][:, a:])
    print(f"x3_layer PS layer {l} {variant}: slice, {int((~ok).sum())} of {ok.numel()} entries differ")
    assert ok.all()
    if l < 5:
        assert torch.equal(part["smax"], full["smax"][:, a:])


@pytest.mark.parametrize("zero_shift", [False, True])
@pytest.mark.parametrize("l,n_win,variant", [c for c in X.PS_CASES if c[1] == 11])
def test_layer_ps_degenerate_samples(l, n_win, variant, zero_shift):
    """Check 5: window 2 all zero (smax_in = 0; with the affine shift t = 0 the bound is 0 too) and, where the input
    carries its mask in the sign bit, window 4 dropped entirely.  Finite, equal to the emulation, and where nothing
    is staged exactly the bias through the ReLU."""
    _ext.require()
    c = X.ps_case(l, n_win, variant, zero_shift=zero_shift)
    r = c["r_in"].clone().view(-1, n_win, 60, c["cin"])
    r[:, 2] = 0.0
    if c["sign_in"]:
        r[:, 4] = -r[:, 4].abs()
    c["r_in"] = r.view(-1, 60, c["cin"])
    c["smax_in"] = X.f32_bits(c["r_in"].abs().amax((1, 2)))
    assert (c["smax_in"].view(-1, n_win)[:, 2] == 0).all()
    res = _run_ps(c)
    _check_against_ref(c, res, f"x3_layer PS layer {l} {variant} degenerate, shift {'0' if zero_shift else 'kept'}")
    if l < 5:
        empty = ([2] if zero_shift else []) + ([4] if c["sign_in"] else [])
        for g in range(GROUPS):
            relu_b = c["bias"][g if c["per_group"] else 0].clamp_min(0.0)
            for w in empty:
                assert torch.equal(res["out"][g, w].abs(), relu_b.expand(60, -1)), f"window {w} of group {g}"
