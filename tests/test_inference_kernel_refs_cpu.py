"""CPU checks of ``tests/inference_kernel_refs.py``: the probe fixtures meet their conditions, the float64 reference
agrees with ``models/reference.py`` and with the fp32 emulations of the packed probes (the packers' test), a
one-grid-unit change of a stored activation is visible in the logit, and every listed mistake moves a logit (or
the entries it touches) by at least 10 allowances.  Each test prints its figures before it asserts; the factors
are recorded in ``profiles/inference_kernel_pins.md``."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import fused, generic

from . import inference_kernel_refs as R

N_WIN = 5          # 2^0 / 2^7 / 2^-9 copies of one window, the zero window, one more
ARITHS = {"nopool": ("fused", "layer"), "pooled": ("fused", "x3", "layer"), "single": ("fused", "x3", "layer")}
KERNEL_OF = {(k, a): name for name, (k, a, _) in R.KERNELS.items()}


def _f64(p):
    return {k: v.double() for k, v in p.items()}


# ================================================================================================ fixtures
@pytest.mark.parametrize("kind", R.KINDS)
def test_probe_fixture_conditions(kind):
    spec = R.probe_spec(kind)
    assert all(R.rows_covered(kind)), "a k-row without a weight in any net"
    for net in range(R.N_NETS):
        p = R.probe_params(kind, net)
        for i in range(1, 7):
            w = p[f"conv1d_{i}/kernel"]
            # at most 11 significant bits: the fp16 lo half of W 2^sw is zero
            fr, _ = fused.pack_conv_fragments_x3(w)
            assert not fr[:, :, 1].any()
            scale, shift = fused.bn_affine(spec, p, i)
            assert torch.equal(scale, p[f"batchnorm_{i}/gamma"]), "the folded scale is not gamma"
            assert (scale < 0).any() and (scale == 0).any() and (scale > 0).any()
            assert ((scale.reshape(-1, 16) != 0).sum(1) >= 8).all()
            assert torch.equal(shift, shift.round()) and shift.abs().max() <= 1
            assert ((w != 0).sum((0, 1)) > 0).all()
        if net == R.N_NETS - 1:
            assert all((p[f"conv1d_{i}/bias"] <= 0).all() and not fused.bn_affine(spec, p, i)[1].any() for i in range(1, 7))
    x = R.probe_windows(kind, N_WIN)
    assert torch.equal(x[1], x[0] * 128) and torch.equal(x[2], x[0] / 512) and not x[3].any()
    assert torch.equal(x.to(torch.bfloat16).float(), x)


def test_conv_cases_cover_the_issue():
    cs = R.conv_cases()
    kern = {R.conv_kernel_of(c) for c in cs}
    assert kern == {"conv_lds_kernel", "conv_block_kernel<true>", "conv_block_kernel<false>"}
    assert R.conv_kernel_of(dict(cin=320, k=3)) == "conv_block_kernel<true>"
    assert {c["cin"] for c in cs} >= {1, 4, 12, 32, 320} and {c["k"] for c in cs} == {1, 3, 9}
    assert {(c["L"], c["pool"]) for c in cs} >= {(7, True), (30, True), (30, False)}
    assert {c["cout"] for c in cs} == {4, 20, 96, 132}
    rows = {c["n"] * ((c["L"] + 1) // 2 * 2 if c["pool"] else c["L"]) for c in cs}
    assert rows >= {8, 120, 136}
    assert {c["n_win"] for c in cs if c["drop"]} >= {1, 3} and any(not c["drop"] for c in cs)
    assert any(c["drop"] and c["n"] // c["n_win"] > 1 and c["n_win"] > 1 for c in cs)
    for k in kern:      # every kernel with and without pool and mask
        sub = [c for c in cs if R.conv_kernel_of(c) == k]
        assert {c["pool"] for c in sub} == {True, False} and {c["drop"] for c in sub} == {True, False}, k


# ================================================================================================ reference
def _rounding_bound(kind, p, r, dropout):
    """Per-logit bound on what the bf16 stores of ``r`` can move: the half-ulp of every stored value, carried
    through |w|, |scale|, the pool and the mask scale (ReLU and max are 1-Lipschitz)."""
    spec = R.probe_spec(kind)
    e = None
    for l, b in enumerate(spec.blocks):
        y = r.acts[l]
        if e is not None:
            s = fused.bn_affine(spec, p, l + 1)[0].double().abs()
            e = R._pad_conv(e, p[f"conv1d_{l + 1}/kernel"].double().abs()) * s
            if b.pool:
                lo = e.shape[1] // 2
                e = torch.maximum(e[:, 0:2 * lo:2], e[:, 1:2 * lo:2])
            if dropout:
                e = e / (1.0 - b.dropout)
        else:
            e = torch.zeros_like(y)
        e = e + R.UB * y.abs()
    return (e * p["output_layer/kernel"].double().reshape(-1).abs()).sum((1, 2)) / r.L


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_matches_model_reference(kind, dropout):
    """x3 probes (no store rounds): equal to ``reference.forward(dtype=float64)`` up to the float64 rounding of
    its mean; bf16 probes: within the bf16 roundings the probe reference applies."""
    spec = R.probe_spec(kind)
    x = R.probe_windows(kind, N_WIN)
    for net in range(R.N_NETS):
        p = R.probe_params(kind, net)
        want = reference.forward(spec, _f64(p), x.double(), dropout=dropout, bn_batch_stats=False, seed=R.SEED,
                                 pass_id=R.PASS_OFF, sample_ids=torch.arange(N_WIN) + R.WIN_OFF, return_logits=True,
                                 dtype=torch.float64).reshape(-1)
        for arith in ARITHS[kind]:
            r = R.probe_reference(kind, arith, N_WIN, 1, dropout, net)
            d = (r.logit - want).abs()
            if arith == "x3":
                assert bool((d <= 1e-13 * (r.Sabs / r.L + 1)).all()), (kind, net, d.max())
            else:
                bound = _rounding_bound(kind, p, r, dropout)
                print(f"{kind} net {net} {arith} dropout {dropout}: |probe - model| / rounding bound "
                      f"{float((d / bound.clamp(min=1e-300)).max()):.3f}")
                assert bool((d <= bound + 1e-13 * (r.Sabs / r.L + 1)).all()), (kind, net, arith)


def _params_from_blob(kind, blob, x3):
    """The network a blob encodes, read back through the unpackers: kernel (x 2^sw for x3), the folded epilogue
    rows as (bias, scale, shift)."""
    spec = R.probe_spec(kind)
    ch = spec.channels()
    lay = fused.layout_x3() if x3 else fused.layout()
    q = {}
    for l, b in enumerate(spec.blocks):
        i, k, cin, cout = l + 1, b.kernel_size, ch[l], b.filters
        nstep = (k * cin + 31) // 32
        if x3:
            nb = 2 * nstep * (cout // 16) * 1024
            fr = blob[lay["woff"][l]: lay["woff"][l] + nb].view(torch.float16).reshape(nstep, cout // 16, 2, 64, 8)
            full = fused.unpack_conv_fragments_x3(fr, 0, 1, nstep * 32, cout).reshape(nstep * 32, cout)
        else:
            nb = nstep * (cout // 16) * 1024
            fr = blob[lay["woff"][l]: lay["woff"][l] + nb].view(torch.bfloat16).reshape(nstep, cout // 16, 64, 8)
            full = fused.unpack_conv_fragments(fr, 1, nstep * 32, cout).reshape(nstep * 32, cout)
        assert not full[k * cin:].any(), "non-zero padding lanes"
        epi = blob[lay["eoff"][l]: lay["eoff"][l] + 32 * cout].view(torch.float32).reshape(8, cout).double()
        assert torch.equal(epi[4:], epi[:4] / (1.0 - b.dropout)), "the 1 / (1 - rate) rows"
        s, tq, lo, hi = epi[0], epi[1], epi[2], epi[3]
        assert bool(torch.where(s >= 0, (hi == float("inf")) & (lo > -float("inf")),
                                (lo == -float("inf")) & (hi < float("inf"))).all()), "the clamp of a negative scale"
        t = torch.where(s >= 0, lo, hi)
        q[f"conv1d_{i}/kernel"] = full[:k * cin].reshape(k, cin, cout).double()
        q[f"conv1d_{i}/bias"] = torch.where(s != 0, (tq - t) / torch.where(s != 0, s, torch.ones_like(s)), torch.zeros_like(s))
        q[f"batchnorm_{i}/gamma"] = s
        q[f"batchnorm_{i}/beta"] = t
        q[f"batchnorm_{i}/moving_mean"] = torch.zeros_like(s)
        q[f"batchnorm_{i}/moving_variance"] = torch.full_like(s, 1.0 - R.BN_EPS)
    head = blob[lay["dense"]: lay["dense"] + 4 * (ch[6] + 1)].view(torch.float32).double()
    q["output_layer/kernel"], q["output_layer/bias"] = head[:ch[6]].reshape(-1, 1), head[ch[6]:]
    return q


@pytest.mark.parametrize("kind", R.KINDS)
def test_packed_probes_encode_the_probe(kind):
    """``pack_blob`` / ``pack_blob_x3`` on the probes: the network read back from the blob (fragments, epilogue
    rows, the [-inf, t] clamp of a negative scale, the 2^-sw fold) gives every stored activation of the reference
    bitwise, with and without dropout."""
    spec = R.probe_spec(kind)
    x = R.probe_windows(kind, N_WIN)
    widx, passes, wins = R.launch_samples(N_WIN, 1, True)
    for net in range(R.N_NETS):
        p = R.probe_params(kind, net)
        for x3 in ((False,) if kind == "nopool" else (False, True)):
            blob = (fused.pack_blob_x3 if x3 else fused.pack_blob)(spec, p)
            q = _params_from_blob(kind, blob, x3)
            for dropout in (False, True):
                arith = "x3" if x3 else "fused"
                want = R.probe_reference(kind, arith, N_WIN, 1, dropout, net)
                got = R.forward64(kind, q, x[widx], passes, wins, arith=arith, dropout=dropout, check=False)
                for l in range(6):
                    assert torch.equal(got.acts[l], want.acts[l]), (kind, net, x3, dropout, l)
                assert torch.equal(got.logit, want.logit)


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp32_emulations_match(kind, dropout):
    """``fused.emulate_blob_forward`` (no-pool blob) and ``generic.emulate`` (both hand-overs) on the probes: fp32
    arithmetic that is exact up to the head, whose ``mean(1) @ w`` rounds once per channel and adds C terms:
    (C + 2) U32 sum |dw y6| / L + U32 |db|."""
    spec = R.probe_spec(kind)
    x = R.probe_windows(kind, N_WIN)
    ids = torch.arange(N_WIN) + R.WIN_OFF
    worst = 0.0
    for net in range(R.N_NETS):
        p = R.probe_params(kind, net)
        runs = [("layer", generic.emulate(spec, p, x, dropout=dropout, seed=R.SEED, pass_id=R.PASS_OFF, sample_ids=ids,
                                          logits=True, last_fp32=False)),
                ("fused", generic.emulate(spec, p, x, dropout=dropout, seed=R.SEED, pass_id=R.PASS_OFF, sample_ids=ids,
                                          logits=True, last_fp32=True))]
        if kind == "nopool":
            runs.append(("fused", fused.emulate_blob_forward(fused.pack_blob(spec, p), x, spec, dropout=dropout, seed=R.SEED,
                                                             pass_id=R.PASS_OFF, sample_ids=ids, logits=True)))
        for arith, got in runs:
            r = R.probe_reference(kind, arith, N_WIN, 1, dropout, net)
            allow = (spec.final_channels + 2) * R.U32 * r.Sabs / r.L + R.U32 * abs(float(r.db))
            worst = max(worst, R.ratio(got.double() - r.logit, allow))
    print(f"{kind} dropout {dropout}: emulations, |err| / allowance {worst:.3f}")
    assert worst <= 1.0


# ================================================================================================ sensitivity
def _sensitivity(kind, arith, net, l, nsamp=150, w=4):
    """Share of ``nsamp`` stored elements of block ``l`` (0-based) of window ``w`` whose change by one grid unit
    moves the logit by >= 10 allowances."""
    kernel = KERNEL_OF[(kind, arith)]
    base = R.probe_reference(kind, arith, N_WIN, 1, False, net)
    p = R.probe_params(kind, net)
    act = base.acts[l][w]
    unit = 2.0 ** -float(R.grid_exp(act[None])[0])
    g = torch.Generator().manual_seed(1000 * R.KINDS.index(kind) + 10 * l + net)
    t = torch.randint(0, act.shape[0], (nsamp,), generator=g)
    c = torch.randint(0, act.shape[1], (nsamp,), generator=g)
    sgn = torch.where(torch.rand(nsamp, generator=g) < 0.5, -1.0, 1.0).double()
    batch = act.repeat(nsamp, 1, 1)
    batch[torch.arange(nsamp), t, c] += sgn * unit
    ids = torch.full((nsamp,), w)
    r = R.forward64(kind, p, batch, ids * 0 + R.PASS_OFF, ids + R.WIN_OFF, arith=arith, check=False, start=l + 1)
    allow = R.head_allow(kernel, base)[w]
    return float(((r.logit - base.logit[w]).abs() >= 10 * allow).double().mean())


@pytest.mark.parametrize("kind", R.KINDS)
def test_one_grid_unit_is_visible(kind):
    """A condition of the fixtures: in every block 1-5, >= 75 % of the stored elements, changed by one grid unit,
    move the logit by >= 10 head allowances."""
    arith = "fused"
    fr = [[_sensitivity(kind, arith, net, l) for l in range(5)] for net in range(R.N_NETS)]
    low = [min(f[l] for f in fr) for l in range(5)]
    print(f"{kind}: share of elements visible at 10 allowances, blocks 1-5 (lowest of {R.N_NETS} nets): "
          + " ".join(f"{100 * v:.0f}%" for v in low))
    assert min(low) >= 0.75, low


# ================================================================================================ mistakes
N_PASS = 3
COMMON = ("tap_first", "tap_last", "halo_one", "leak_prev", "tile_swap", "pad_lanes")
MASKS = ("slot_key", "mask_layer", "mask_pass")
POOLED = ("mask_unpooled", "pool_shift", "pool_before_affine")


def _fault_factor(kind, arith, fault, block, dropout):
    kernel = KERNEL_OF[(kind, arith)]
    x = R.probe_windows(kind, N_WIN)
    widx, passes, wins = R.launch_samples(N_WIN, N_PASS, dropout)
    worst = 0.0
    for net in range(R.N_NETS):
        p = R.probe_params(kind, net)
        base = R.probe_reference(kind, arith, N_WIN, N_PASS, dropout, net)
        nb = None
        if fault == "x3_neighbour":
            e = R.x3_exp(base.acts[block - 1])
            idx = torch.arange(len(e))
            nb = (e, e[torch.where(idx + 1 < len(e), idx ^ 1, idx).clamp(max=len(e) - 1)])
        bad = R.forward64(kind, p, x[widx], passes, wins, arith=arith, dropout=dropout, check=False, fault=fault,
                          fault_block=block, neighbour=nb)
        worst = max(worst, R.ratio(bad.logit - base.logit, R.head_allow(kernel, base)))
    return worst


def _faults(kind):
    out = [(f, 0 if f == "pad_lanes" else 1, False) for f in COMMON] + [(f, 1, True) for f in MASKS]
    if kind == "pooled":
        out += [("mask_unpooled", 1, True), ("pool_shift", 1, False), ("pool_before_affine", 1, False)]
    else:
        out += [("gap64", 5, False)]
    return out


@pytest.mark.parametrize("kind", R.KINDS)
def test_allowances_catch_mistakes(kind):
    """Each mistake, applied to the reference (block 2 unless it belongs elsewhere), moves at least one sample's
    logit by >= 10 head allowances."""
    for fault, block, dropout in _faults(kind):
        for arith in [a for a in ARITHS[kind] if a != "layer"]:
            f = _fault_factor(kind, arith, fault, block, dropout)
            print(f"{kind} {arith} {fault}: {f:.3g} allowances")
            assert f >= 10, (kind, arith, fault, f)
    if kind != "nopool":
        f = _fault_factor(kind, "x3", "x3_neighbour", 1, False)
        print(f"{kind} x3 x3_neighbour: {f:.3g} allowances")
        assert f >= 10


def test_conv_allowance_catches_mistakes():
    """generic_conv: ``n / n_win`` taken as the window moves >= 10 allowances (or a mask zero) on the share of
    entries it touches; a store of channels ``cout .. cout_pad - 1`` lands outside the (n, Lout, cout) tensor --
    on the next row's first channels, where the reference holds other values."""
    cs = R.conv_cases()
    hit = 0
    for idx, c in enumerate(cs):
        fx = R.conv_fixture(c, idx)
        ref, allow, keep = R.conv_ref(c, fx)
        if c["drop"] and c["n_win"] > 1 and c["n"] // c["n_win"] > 1:
            bad, _, kb = R.conv_ref(c, fx, fault="win_is_pass")
            touched = keep != kb
            share = float(((bad - ref).abs()[touched] >= 10 * allow[touched]).double().mean())
            print(f"case {idx}: window / pass swapped: {100 * float(touched.double().mean()):.0f}% of the entries "
                  f"touched, {100 * share:.0f}% of them by >= 10 allowances")
            # a touched entry moves by its whole value: visible unless the value itself is within 10 allowances of 0
            assert float(touched.double().mean()) > 0.2 and share >= 0.9
            hit += 1
        cpad = fx["cpad"]
        if cpad > c["cout"]:
            # the padded channels' values (acc = 0: clamp(t') of the zero-padded rows = 0) written past the row
            flat = ref.reshape(-1, c["cout"])
            if flat.shape[0] > 1:
                over = flat[1:, : cpad - c["cout"]]
                a = allow.reshape(-1, c["cout"])[1:, : cpad - c["cout"]]
                share = float(((over - 0.0).abs() >= 10 * a)[over != 0].double().mean())
                print(f"case {idx}: padded-channel store: {100 * share:.0f}% of the overwritten entries by >= 10 allowances")
                # an entry within 10 allowances of zero cannot show the zero written over it
                assert share >= 0.75
    assert hit >= 1


def test_generic_head_allowance_catches_mistakes():
    for (L, C) in R.HEAD_SHAPES:
        y, w, b = R.head_fixture(L, C, 5, False)
        z, a_z, p, a_p = R.generic_head_ref(y, w, b)
        if L > 1:   # the mean over L + 1 rows, a row of the next sample added
            bad = (y.double() * w.double()).sum((1, 2)) / (L + 1) + b
            f = R.ratio(bad - z, a_z)
            print(f"generic_head ({L}, {C}): 1 / (L + 1): {f:.3g} allowances")
            assert f >= 10
        bad = z - (y.double()[:, L - 1] * w.double()).sum(1) / L      # the last row left out
        f = R.ratio(bad - z, a_z)
        print(f"generic_head ({L}, {C}): the last row left out: {f:.3g} allowances")
        assert f >= 10
