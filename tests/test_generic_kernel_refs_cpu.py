"""The float64 oracle of the generic training kernels (``tests/generic_kernel_refs.py``) checked where no
GPU is needed:

* composed into a whole training step, the per-kernel references reproduce float64 autograd over
  ``models/reference.py:forward`` (same masks) to 1e-9: loss, every gradient, the moving statistics;
* every allowance formula is far below the error of a real mistake -- the last row of the last sample
  dropped, one tap shifted by a row, the mask of ``window_offset + 1``, the pool winner swapped on one pair,
  ``out_off`` off by one, one slot of a slot table skipped: the largest deviation is at least 10 times its
  allowance on every shape the GPU file uses;
* the pool pairs left out of the backward comparison (unequal z, float64 values within 2^-20): none for
  bf16 storage, at most 1e-3 of the pairs for fp32, on the fixtures themselves."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng

from . import generic_kernel_refs as G
from .test_generic_gpu import SPECS

POWER = 10.0


def _ratio(dev, allow):
    """Largest |deviation| / allowance (a zero allowance under a non-zero deviation counts as infinite)."""
    dev, allow = dev.abs().reshape(-1), allow.reshape(-1)
    r = torch.where(allow > 0, dev / allow.clamp(min=1e-300), torch.where(dev > 0, torch.full_like(dev, float("inf")),
                                                                          torch.zeros_like(dev)))
    return float(r.max())


# ------------------------------------------------------------------------------------------ composition
def compose_step(spec, p, x, y, seed, pass_id):
    """One training step built from the per-kernel references, float64 throughout (no bf16 rounding)."""
    n, lens, nl = x.shape[0], spec.lengths(), len(spec.blocks)
    h, S, stats, g = x, [], {}, {}
    for l, b in enumerate(spec.blocks):
        i, L = l + 1, lens[l]
        w, bias = p[f"conv1d_{i}/kernel"], p[f"conv1d_{i}/bias"]
        u = G.conv64(h, w, bias, relu=True)
        sc, sh, mean, rstd, mm, mv = G.bn_finalize64(
            G.moments64(u)[None], 1.0 / (n * L), p[f"batchnorm_{i}/gamma"], p[f"batchnorm_{i}/beta"], spec.bn_epsilon,
            spec.bn_momentum, p[f"batchnorm_{i}/moving_mean"], p[f"batchnorm_{i}/moving_variance"])
        stats[f"batchnorm_{i}/moving_mean"], stats[f"batchnorm_{i}/moving_variance"] = mm, mv
        lout = L // 2 if b.pool else L
        keep = G.keep_mask(rng.stream_key(seed, l, pass_id), 0, n, lout, b.filters, b.dropout) if b.dropout > 0 else None
        ik = 1.0 / (1.0 - b.dropout)
        win = G.pool_winner(u, sc, sh, False)[0] if b.pool else None
        S.append((h, u, mean, rstd, keep, ik, win))
        h = G.apply64(u, sc, sh, b.pool, keep, ik)[0]
    wd = p["output_layer/kernel"].reshape(-1)
    hd = G.head64(h, wd, p["output_layer/bias"], y, 1.0 / n)
    g["output_layer/kernel"], g["output_layer/bias"] = hd["gw"].reshape(-1, 1), hd["gb"].reshape(1)
    up = G.head_upstream64(hd["dlog"], wd, 1.0 / h.shape[1], h.shape[1])
    for l in range(nl - 1, -1, -1):
        i, b, L = l + 1, spec.blocks[l], lens[l]
        hin, u, mean, rstd, keep, ik, win = S[l]
        dy = G.upstream64(up, L, b.pool, keep, ik, win)
        sums, _ = G.bwd_stats64(u, mean, rstd, dy)
        g[f"batchnorm_{i}/gamma"], g[f"batchnorm_{i}/beta"], coef = G.bwd_finalize64(sums, 1.0 / (n * L))
        dz, _ = G.bwd_dz64(u, mean, rstd, p[f"batchnorm_{i}/gamma"], dy, coef[0], coef[1])
        g[f"conv1d_{i}/bias"] = dz.sum((0, 1))
        # wgrad in the padded row layout of ops/generic_train.py: x row (s, t) at s rs + 2 p + t, dz at s rs + p + t
        k = b.kernel_size
        pd = (k - 1) // 2
        rs = L + 2 * pd
        xp = G.place_rows(torch.zeros(2 * pd + n * rs, hin.shape[2], dtype=torch.float64), hin, rs, 2 * pd)
        dzp = G.place_rows(torch.zeros(n * rs, dz.shape[2], dtype=torch.float64), dz, rs, pd)
        g[f"conv1d_{i}/kernel"] = G.wgrad64(xp, dzp, n * rs, k)[0]
        if l > 0:
            up = G.conv64(dz, G.flip_t(p[f"conv1d_{i}/kernel"]))
    return hd["loss"], g, stats


@pytest.mark.parametrize("name", list(SPECS))
def test_composed_references_match_float64_autograd(name):
    spec, n, seed, pass_id = SPECS[name], 5, 11, (1 << 30) + 3
    p = {k: v.double() for k, v in R.synthetic_params(spec, 9).items()}
    gen = torch.Generator().manual_seed(4)
    for k in p:
        if k.endswith("/bias"):
            p[k] = torch.randn(p[k].shape, generator=gen, dtype=torch.float64) * 0.1
    x = torch.randn(n, spec.input_length, spec.input_channels, generator=gen, dtype=torch.float64)
    y = (torch.rand(n, generator=gen) > 0.5).double()
    loss, g, stats = compose_step(spec, {k: v.clone() for k, v in p.items()}, x, y, seed, pass_id)
    q = {k: v.clone().requires_grad_(not k.startswith("batchnorm") or k.endswith(("gamma", "beta"))) for k, v in p.items()}
    logits = R.forward(spec, q, x, dropout=True, bn_batch_stats=True, update_moving=True, seed=seed, pass_id=pass_id,
                       sample_ids=torch.arange(n), return_logits=True, dtype=torch.float64)
    lv = torch.nn.functional.binary_cross_entropy_with_logits(logits.reshape(-1), y, reduction="none")
    lv.mean().backward()
    assert abs(float(loss) - lv.sum().item()) <= 1e-9 * lv.sum().item()
    for k, v in g.items():
        ref = q[k].grad
        assert float((v.reshape(ref.shape) - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), k
    for k, v in stats.items():
        assert float((v - q[k].detach()).abs().max()) <= 1e-9 * float(q[k].detach().abs().max()), k


# ------------------------------------------------------------------------------------------ allowance power
def _tap_shift(x, w, tap):
    """conv(x, w) with tap ``tap`` reading the row after the one it should (zero past the sample's end)."""
    only = torch.zeros_like(w)
    only[tap] = w[tap]
    xs = torch.zeros_like(x)
    xs[:, :-1] = x[:, 1:]
    return G.conv64(x, w) - G.conv64(x, only) + G.conv64(xs, only)


@pytest.mark.parametrize("cin,L,k,cout,n", G.CONV_CASES)
def test_conv_allowances_catch_mistakes(cin, L, k, cout, n):
    x, w, b, dz = G.conv_fixture(cin, L, k, cout, n)
    wb = w.bfloat16().float()
    K = k * cin
    lin = G.conv64(x, wb, b)
    ref, ab = torch.relu(lin), G.conv_abs64(x, wb, b)
    allow = G.conv_allow(ref, ab, K, True)
    # the last row of the last sample never written (the buffer's previous content: zero here)
    drop = ref.clone()
    drop[-1, -1] = 0
    assert _ratio(drop - ref, allow) >= POWER
    # one tap shifted by a row (L = 1: the tap reads nothing)
    mut = torch.relu(_tap_shift(x, wb, k // 2) + b.double())
    assert _ratio(mut - ref, allow) >= POWER
    # moments: one slot of the table skipped -- deterministic mode: the first 64 rows; atomic mode: the row
    # blocks 0, 16, .. of 128 rows
    rows = n * L
    e = G.conv_allow(ref, ab, K, False)
    u = ref.reshape(rows, cout)
    for det in (True, False):
        a = G.moments_allow(ref, e, G.conv_chain(rows, det))
        r = torch.arange(rows)
        gone = (r < 64) if det else ((r // 128) % 16 == 0)
        dev = G.moments64(u[gone])
        assert _ratio(dev, a) >= POWER, det
    # dgrad (mode 2): the same formula on the flipped, transposed kernel
    if cin % 4 == 0:
        wf = G.flip_t(wb)
        dref, dab = G.conv64(dz, wf), G.conv_abs64(dz, wf)
        dallow = G.conv_allow(dref, dab, k * cout, True)
        drop = dref.clone()
        drop[-1, -1] = 0
        assert _ratio(drop - dref, dallow) >= POWER
        assert _ratio(_tap_shift(dz, wf, k // 2) - dref, dallow) >= POWER


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("cin,L,k,cout", G.GF_CASES)
def test_gf_allowances_catch_mistakes(cin, L, k, cout, scale):
    n = 9
    x, w, b, dz = G.conv_fixture(cin, L, k, cout, n)
    x, b, dz = x * scale, b * scale, dz * scale
    lin = G.conv64(x, w, b)
    ref, ab = torch.relu(lin), G.conv_abs64(x, w, b)
    allow = G.conv_allow(ref, ab, k * cin, False)
    drop = ref.clone()
    drop[-1, -1] = 0
    assert _ratio(drop - ref, allow) >= POWER
    assert _ratio(torch.relu(_tap_shift(x, w, k // 2) + b.double()) - ref, allow) >= POWER
    rows = n * L
    for det in (True, False):
        a = G.moments_allow(ref, allow, G.conv_chain(rows, det))
        r = torch.arange(rows)
        gone = (r < 64) if det else ((r // 128) % 16 == 0)
        assert _ratio(G.moments64(ref.reshape(rows, cout)[gone]), a) >= POWER, det
    pd, rs = (k - 1) // 2, L + k - 1
    xp = G.place_rows(torch.zeros(2 * pd + n * rs, cin, dtype=torch.float64), x.double(), rs, 2 * pd)
    dzp = G.place_rows(torch.zeros(n * rs, cout, dtype=torch.float64), dz.double(), rs, pd)
    _check_wgrad_power(xp, dzp, n * rs, k, 2)


def _check_wgrad_power(xp, dzp, R, k, extra):
    gw, ab = G.wgrad64(xp, dzp, R, k)
    allow = G.wgrad_allow(ab, R, extra)
    last = int(dzp[:R].abs().sum(1).nonzero().max())   # the last row that carries data
    cut = dzp.clone()
    cut[last] = 0
    assert _ratio(G.wgrad64(xp, cut, R, k)[0] - gw, allow) >= POWER
    # one tap reads the rows one further down
    shifted = gw.clone()
    t = k // 2
    shifted[t] = xp.double()[t + 1: t + R].t() @ dzp.double()[: R - 1] if R > 1 else gw[t] * 0
    assert _ratio(shifted - gw, allow) >= POWER


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("C,L,n", G.HEAD_CASES)
def test_head_allowances_catch_mistakes(C, L, n, bf16):
    """prob / dlog: the last row of the last sample left out of its average.  The batch sums (loss, dense
    gradients): the record of the last workgroup (4 samples) skipped -- the head's slot table."""
    h, w, y = G.head_fixture(C, L, n, bf16)
    cut = h.clone()
    cut[-1, -1] = 0
    b = torch.tensor([G.HEAD_BIASES[0]], dtype=torch.float64)
    # (at the planted +-30 nothing can show a mistake: a saturated sigmoid, and with it the loss of a correctly
    # labelled sample and every gradient, no longer depends on the logit; those calls reach the kernel's
    # saturated branches, they do not add sensitivity)
    ref, mut = G.head64(h, w, b, y, 1.0 / n), G.head64(cut, w, b, y, 1.0 / n)
    allow = G.head_allow(ref, n, C, 1.0 / n)
    for key in ("prob", "dlog"):
        assert _ratio(mut[key] - ref[key], allow[key]) >= POWER, key
    m = 4 * ((n + 3) // 4 - 1)
    part = G.head64(h[:m], w, b, y[:m], 1.0 / n) if m else {k: torch.zeros_like(ref[k]) for k in ("loss", "gw", "gb")}
    for key in ("loss", "gw", "gb"):
        assert _ratio(part[key] - ref[key], allow[key]) >= POWER, key


@pytest.mark.parametrize("cin,k,cout,n,L", G.WGRAD_CASES)
def test_wgrad_allowance_catches_mistakes(cin, k, cout, n, L):
    xp, dzp, R = G.wgrad_fixture(cin, k, cout, n, L)
    _check_wgrad_power(xp.double(), dzp.double(), R, k, 16)


@pytest.mark.parametrize("C", G.BN_C)
@pytest.mark.parametrize("nslots", G.BN_NSLOTS)
def test_bn_finalize_allowances_catch_a_skipped_slot(nslots, C):
    for count in G.BN_COUNTS:
        slots, gamma, beta, mmean, mvar = G.bn_fixture(nslots, C, count)
        args = (1.0 / count, gamma, beta, G.EPS, G.MOMENTUM, mmean, mvar)
        ref, allow = G.bn_finalize64(slots, *args), G.bn_finalize_allow(slots, *args)
        skip = slots.clone()
        skip[nslots - 1] = 0   # the one-slot tail of the packed sum, where there is one
        mut = G.bn_finalize64(skip, *args)
        live = torch.arange(C) != 0   # the all-zero channel has nothing to lose
        for name, r, m, a in zip(("scale", "shift", "mean", "rstd", "mmean", "mvar"), ref, mut, allow):
            assert _ratio((m - r)[live], a[live]) >= POWER, (name, count)
        if nslots >= 255:   # the planted near-constant channels keep a positive variance in the table
            var = G.bn_moments64(slots, 1.0 / count)[1]
            assert float(var[2]) > 2e-5 and float(var[3]) > 2e-7, (count, var[2:4])


def _elem_cases():
    return [(bf16, C, n, L) for bf16 in (True, False) for C in G.ELEM_C for (n, L) in G.ELEM_NL] + G.ELEM_EXTRA


@pytest.mark.parametrize("bf16,C,n,L", _elem_cases())
def test_elementwise_allowances_and_pool_exclusions(bf16, C, n, L):
    rows = n * L
    for vi, (pool, rate, woff) in enumerate(G.elem_variants(bf16, C, n, L)):
        F = G.elem_fixture(bf16, C, n, L, pool, rate, woff, head=bool(vi & 1))
        z, (sc, sh, mean, rstd) = F["z"], F["bn"]
        lout = F["lout"]
        # ---- pool-winner exclusions on the fixture itself
        if pool and lout > 0:
            share = float(F["excl"].double().mean())
            assert share == 0.0 if bf16 else share <= 1e-3, share
            za, zb = G.pool_pairs(z)
            assert int(((za == zb) & (za != 0)).sum()) > 0   # planted non-zero ties are there and compared
        if lout == 0:
            continue
        # ---- gt_apply
        a_y = G.apply_allow(F["y"], F["ymag"], bf16)
        if rate > 0:   # the mask of window_offset + 1
            y2 = G.apply64(z, sc, sh, pool, G.keep_mask(G.SKEY, woff + 1, n, lout, C, rate), F["ik"])[0]
            assert _ratio(y2 - F["y"], a_y) >= POWER
        # out_off off by one: every row holds its neighbour's values (the first the sentinel's)
        flat = F["y"].reshape(n * lout, C)
        off1 = torch.cat([torch.full((1, C), 1e30, dtype=torch.float64), flat[:-1]])
        assert _ratio(off1 - flat, a_y.reshape(n * lout, C)) >= POWER
        drop = flat.clone()
        drop[-1] = 1e30   # last row of the last sample not written: the sentinel stays
        assert _ratio(drop - flat, a_y.reshape(n * lout, C)) >= POWER
        # ---- gt_bwd dz and sums
        a_dz = G.dz_allow(F["dz"], F["dzmag"], bf16)
        live = F["dzmag"] > 0
        if pool:   # the winner swapped on the first pair that carries a gradient
            up = F["dy"][:, 0: 2 * lout: 2] + F["dy"][:, 1: 2 * lout: 2]
            idx = (up.abs() * ((G.pool_pairs(z)[0] > 0) | (G.pool_pairs(z)[1] > 0))).reshape(-1).argmax()
            win2 = F["win"].clone().reshape(-1)
            win2[idx] = ~win2[idx]
            g = F["dh"] if "dh" in F else G.head_upstream64(F["dlog"], F["w"], F["invL"], lout).expand(n, lout, C)
            dy2 = G.upstream64(g, L, True, F["keep"], F["ik"], win2.reshape(F["win"].shape))
            dz2 = G.bwd_dz64(z, mean, rstd, F["gamma"], dy2, F["coef"][0], F["coef"][1])[0]
            if bool(live.any()):
                assert _ratio(dz2 - F["dz"], torch.maximum(a_dz, G.dz_allow(dz2, G.bwd_dz64(
                    z, mean, rstd, F["gamma"], dy2, F["coef"][0], F["coef"][1])[1], bf16))) >= POWER
        if bool(live.any()):
            shift = torch.cat([torch.full((1, C), 1e30, dtype=torch.float64), F["dz"].reshape(rows, C)[:-1]])
            assert _ratio(shift - F["dz"].reshape(rows, C), a_dz.reshape(rows, C)) >= POWER
        # one slot of the backward sums skipped: atomic (16 slots) and deterministic (256 slots; 16: capped grid)
        rpb = 256 // (C // 4)
        for det, slots in ((False, 16), (True, 256), (True, 16)):
            grid = G.elem_grid(rows, rpb * 4)
            grid = min(grid, slots) if det else grid
            blk = (torch.arange(rows) // rpb) % grid
            gone = (blk == 0) if det else (blk % 16 == 0)
            chain = G.bwd_chain(rows, C, slots, det)
            dev, _ = G.bwd_stats64(z.reshape(1, rows, C)[:, gone], mean, rstd, F["dy"].reshape(1, rows, C)[:, gone])
            has = F["sums_abs"] > 0
            if bool(has.any()):
                assert _ratio(dev[has], (chain * G.U32 * F["sums_abs"])[has]) >= POWER, (det, slots)


def test_case_tables_reach_every_path():
    """The dispatch decisions the case comments name, read from the launch plans (csrc/generic_geo.h)."""
    wg = {(cin, k, cout): G.geo_table("gt_wgrad", n * (L + k - 1), cin, cout, k, 0, 0) for cin, k, cout, n, L in G.WGRAD_CASES}
    nco = {c: t["nco"] for c, t in wg.items()}
    assert set(nco.values()) == {1, 2, 3, 4}
    assert nco[96, 5, 256] == 4 and nco[224, 9, 192] == 3 and nco[100, 9, 256] == 2 and nco[96, 15, 256] == 2
    assert [nco[c[:3]] for c in G.WGRAD_CASES] == [1, 1, 2, 2, 1, 1, 4, 3, 2, 1, 2]      # as the case comments say
    assert {t["kmax"] for t in wg.values() if not t["im2col"]} == {3, 5, 9, 15}
    assert [c[:3] for c in G.WGRAD_CASES if wg[c[:3]]["im2col"]] == [(1, 7, 12), (3, 9, 20), (4, 7, 100)]
    assert wg[36, 3, 100]["rgs"] == 3 and wg[36, 3, 100]["chunks"] == 9 and wg[1, 7, 12]["rgs"] == 1

    plans = [G.geo_table("conv", G.BF16, G.TRAIN, n, L, cin, (cout + 15) // 16 * 16, k, 0, L + k - 1)
             for cin, L, k, cout, n in G.CONV_CASES]     # gt_conv mode 1: in_rs = L + 2 p
    assert [p["kind"] for p in plans] == ["staged"] * 5 + ["vec"] * 2 + ["elem"] * 4
    # "70.5 KB of LDS (just under the 80 KB limit)", "LDS span 97.5 KB", "LDS span 462 KB"
    assert plans[2]["lds_bytes"] == 70528 and plans[2]["lds_limit_bytes"] == 80 * 1024
    assert [p["span"] * p["lds_stride"] / 1024 for p in plans[5:7]] == [97.5, 462.0]
    assert [p["grid"][1] for p in plans] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1]
    assert sum((cout + 15) // 16 > 8 for _, _, _, cout, _ in G.CONV_CASES) == 2   # second channel block
    # packed slot sum from 256 slots; the one-slot tail joins the previous range
    assert [s for s in G.BN_NSLOTS if s >= 256 and s % 64 == 1] == [257, 321, 385]
    # capped grid of a 16-slot deterministic backward table
    for C, rows in ((4, 18000), (1024, 405), (256, 405)):
        assert G.elem_grid(rows, 256 // (C // 4) * 4) > 16
