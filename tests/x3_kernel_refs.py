"""float64 CPU references of the x3 engine's kernels, one kernel each (``csrc/x3_layers.hip``: ``l1_kernel``,
``aff_kernel``, ``head_kernel`` and the ``PS = true`` variants of ``layer_kernel``), the allowances they are
compared under and the fixtures both test files share (``test_x3_kernel_refs_cpu.py`` checks this oracle
without a GPU, ``test_x3_kernels_gpu.py`` holds the kernels to it).

Every reference works on the kernel's ACTUAL inputs (the fp32 values it reads, upcast to float64), so what is
left between kernel and reference is the kernel's own rounding.  ``U32 = 2^-23`` per fp32 operation (twice
the unit roundoff, ``tests/generic_kernel_refs.py``).

* ``x3_l1``: an output entry is a chain of 28 fp32 FMAs started at the bias, then the store's ReLU: allowance
  ``(28 + 2) U32 (|x| conv |w| + |b|)``.  Moment sums: a thread adds the 30 steps of its half of up to 8 windows
  into one fp32 ``s1`` / ``s2``, a chain of 30 * 8 = 240 fp32 additions (each at most U32 / 2 of the running sum,
  all terms >= 0: at most 120 U32 of the sum in the worst case); the two halves, the slot and the sum over slots
  are fp64.  The allowance ``L1_MOMENT_CHAIN U32 sum`` with ``L1_MOMENT_CHAIN = 60 + 8 + 2 = 70`` is tighter
  than that worst case (a rounding error does not take the same sign 240 times) and is held as it is.
* ``x3_aff``: ``tests/generic_kernel_refs.py:bn_finalize_allow``'s derivation with the kernel's operations:
  var -> fp32, var + eps, sqrtf, the division and ``* dsc`` are (1/2 + 1/2 + 1 + 1 + 1) 2^-24 = 2^-22 of the
  scale, allowed 2^-21; the shift carries the scale's error on ``mean sc`` and two roundings of its own:
  2^-21 (|beta| + |mean sc|) dsc.  The fp64 cancellation of E[u^2] - mean^2 (2^-50 E[u^2], relative to
  var + eps, halved by the square root) is carried into both.  A subnormal result may be off by one
  subnormal step per rounding, 2^-149 each.  Moving update: 2^-22 of the absolute terms per application (two
  fp32 roundings), plus the fp32 rounding of the batch mean / variance it reads, summed over applications.
* ``x3_head``: 2 ceil(C / 64) operations per lane (a product and an addition per channel), 6 steps of the
  wave sum, and 4 for the roundings inside one term (the two affine products, their sum, ``* 1/60``).
"""
import math

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng, x3

from . import generic_kernel_refs as G
from . import test_x3_rowdesc_gpu as RD

U32 = G.U32
EPS, MOMENTUM = G.EPS, G.MOMENTUM
SLOTS = x3.STAT_SLOTS
L = 60
TINY = 2.0 ** -149                    # one fp32 subnormal step
SCALE_EXPS = (0, 12, -18, 5, -7)      # window i of a mixed-scale case is scaled by 2^SCALE_EXPS[i % 5]
BOUNDARY = 2.0 ** -18                 # fixtures keep their prescale bounds this far (relative) from a power of two
GROUPS, GRID, SEED, PASS_BASE, WIN_OFF = RD.GROUPS, RD.GRID, RD.SEED, RD.PASS_BASE, RD.WIN_OFF
REL_BOUND, MOMENT_RTOL = RD.REL_BOUND, RD.MOMENT_RTOL
DSC = float(np.float32(1.0 / 0.7))    # the kernels take dsc as float


def f32_bits(t):
    """fp32 tensor -> its bit patterns (int32): the layout of the smax buffers."""
    return t.float().contiguous().view(torch.int32)


def bits_f32(t):
    return t.contiguous().view(torch.float32)


def ratio(dev, allow):
    """Largest |deviation| / allowance; a non-finite deviation, or a non-zero one under a zero allowance, is inf."""
    dev, allow = dev.abs().reshape(-1).double(), allow.reshape(-1).double()
    inf = torch.full_like(dev, float("inf"))
    r = torch.where(allow > 0, dev / allow.clamp(min=1e-300), torch.where(dev > 0, inf, torch.zeros_like(dev)))
    r = torch.where(torch.isfinite(dev), r, inf)
    return float(r.max())


# ------------------------------------------------------------------------------------------ prescale exponent
def prescale_exp(bound):
    """``csrc/f16x3.h:prescale_exp`` on a tensor: clamp(14 - e, +-100), bound = f 2^e with f in [0.5, 1); e = 0
    for a bound that is 0, negative or not finite."""
    bound = bound.double()
    e = torch.frexp(bound)[1].long()
    e = torch.where((bound > 0) & torch.isfinite(bound), e, torch.zeros_like(e))
    return (14 - e).clamp(-100, 100)


def near_pow2(bound):
    """True where a positive bound is within ``BOUNDARY`` (relative) of a power of two: there the kernel's fp32
    bound may land on the other side, so fixtures must not have such bounds (asserted on the CPU)."""
    bound = bound.double()
    f = torch.frexp(bound)[0]          # [0.5, 1)
    return (bound > 0) & torch.isfinite(bound) & ((f < 0.5 * (1 + BOUNDARY)) | (f > 1 - BOUNDARY))


def sample_prescale_ref(amax, rmax):
    """``sample_prescale``: prescale_exp(fp32(amax0 rmax + amax1)) per sample -> (sa (n,) int64, the float64 bound).
    The float64 product of two fp32 values is exact, so one rounding of the sum to fp32 is the kernel's fma."""
    b64 = amax[0].double() * rmax.double() + amax[1].double()
    return prescale_exp(b64.float()), b64


# ------------------------------------------------------------------------------------------ block 1
L1_NWIN = [1, 7, 8, 9, 137]
L1_MOMENT_CHAIN = 60 + 8 + 2


def l1_halo_windows(n_win):
    return sorted({n_win - 1} | ({3} if n_win > 4 else set()))


def l1_fixture(n_win, groups, all_zero=False):
    """x (n_win, 60, 4), w (groups, 7, 4, 128), b (groups, 128), distinct per group.  The halo windows have their
    first and last three steps large and the rest zero; window 0 (n_win >= 2) is all zero; the last group's bias
    is all negative, so that group's output of the zero window is all zero and its smax 0.  ``all_zero``: every
    window zero (the n_win = 1 form of the zero window)."""
    g = G._gen(31, n_win, groups)
    x = torch.randn(n_win, L, 4, generator=g)
    for w in l1_halo_windows(n_win):
        e = 50.0 * torch.randn(6, 4, generator=g)
        x[w] = 0.0
        x[w, :3], x[w, -3:] = e[:3], e[3:]
    if n_win >= 2:
        x[0] = 0.0
    if all_zero:
        x.zero_()
    w = torch.randn(groups, 7, 4, 128, generator=g) / math.sqrt(28.0)
    b = 0.2 * torch.randn(groups, 128, generator=g)
    b[-1] = -b[-1].abs() - 0.01
    return x.float(), w.float(), b.float()


def l1_ref(x, w, b, conv=G.conv64):
    """-> (R_1 (groups, n_win, 60, 128) float64, its per-entry allowance).  ``conv(x, w[g])``: the product
    before the bias (the CPU tests put a mutated one here)."""
    ys = torch.stack([(conv(x, w[g]) + G.f64(b[g])).clamp_min(0.0) for g in range(w.shape[0])])
    al = torch.stack([(28 + 2) * U32 * G.conv_abs64(x, w[g], b[g]) for g in range(w.shape[0])])
    return ys, al


def stored_moments(out):
    """(groups, 2, C) float64 sums of the stored outputs (groups, n, 60, C) and of their squares."""
    r = out.double().abs()
    return torch.stack([r.sum((1, 2)), (r * r).sum((1, 2))], 1)


def l1_moment_allow(msum):
    """Every term is >= 0, so the sum of the absolute terms is the sum itself."""
    return L1_MOMENT_CHAIN * U32 * msum


def window_max_bits(out):
    """(groups, n) int32: the bits of the max over each window's stored |outputs|."""
    return f32_bits(out.abs().amax((2, 3)))


# ------------------------------------------------------------------------------------------ BN affine
AFF_C = [1, 96, 224, 256, 300]
AFF_LAYOUTS = [(1, 0), (3, 0), (3, None)]        # (groups, p_gstride); None: C
AFF_MODES = ["batch", "batch_gscale", "update1", "update5", "moving", "moving_amax", "running_gscale"]
AFF_EXTREMES = ["zero", "tiny", "huge"]
AFF_COUNT = 3840


def aff_mode(mode):
    """-> dict(stats, update, repeat, amax, gscale, running) of a mode name."""
    return dict(stats=mode not in ("moving", "moving_amax"), update=mode.startswith("update"),
                repeat=5 if mode == "update5" else 1, amax=mode == "moving_amax", gscale=mode.endswith("gscale"),
                running=mode == "running_gscale")


def aff_fixture(C, groups, p_gstride, kind="ordinary"):
    """Slot sums of ``AFF_COUNT`` real fp32 samples per group and the BN parameters ((groups or 1, C) fp32).
    Channel c of group g is special for c + g < 4: 0 near constant (mean 100, std 0.01), 1 constant (variance 0),
    2 all zero, 3 mean 5 / std 1e-3; the rest relu(N(0.3, 1)) at mixed scales, times (1 + g).  The samples go into
    five slots picked at random, in runs of unequal length.  ``kind``: "zero" -- all-zero stats, beta = 0 and moving
    mean 0 (a bound of 0); "tiny" / "huge" -- bounds of about 1e-35 / 1e35 (both clamps of the exponent)."""
    gen = G._gen(32, C, groups, p_gstride, AFF_EXTREMES.index(kind) + 1 if kind != "ordinary" else 0)
    pg = groups if p_gstride else 1
    stats = torch.zeros(groups, SLOTS, 2, C, dtype=torch.float64)
    for g in range(groups):
        wide = 0.25 + 4 * torch.rand(C, generator=gen)
        # the extremes keep every channel's scale in [1, 1.5] (1 + g), so that the bound stays inside fp32
        u = torch.relu(torch.randn(AFF_COUNT, C, generator=gen) + 0.3) * (wide if kind == "ordinary" else 1 + wide / 8.5) * (1 + g)
        if kind == "ordinary":
            for c in range(C):
                k = c + g
                if k == 0:
                    u[:, c] = 100.0 + 0.01 * torch.randn(AFF_COUNT, generator=gen)
                elif k == 1:
                    u[:, c] = 0.75
                elif k == 2:
                    u[:, c] = 0.0
                elif k == 3:
                    u[:, c] = 5.0 + 1e-3 * torch.randn(AFF_COUNT, generator=gen)
        elif kind == "zero":
            u.zero_()
        u = u.float().double()
        cuts = [0] + sorted(torch.randint(1, AFF_COUNT, (4,), generator=gen).tolist()) + [AFF_COUNT]
        slots = torch.randperm(SLOTS, generator=gen)[:5].tolist()
        for s, a, b in zip(slots, cuts[:-1], cuts[1:]):
            stats[g, s, 0] += u[a:b].sum(0)
            stats[g, s, 1] += (u[a:b] * u[a:b]).sum(0)
    gamma = 0.5 + torch.rand(pg, C, generator=gen)
    beta = 2 * torch.rand(pg, C, generator=gen) - 1
    mmean = torch.randn(pg, C, generator=gen)
    mvar = 0.5 + torch.rand(pg, C, generator=gen)
    if kind == "zero":
        beta.zero_()
        mmean.zero_()
    elif kind == "tiny":
        # bound about 81 gamma, 4e-36 .. 7e-35: the smallest at which gamma / sqrt(var + eps) stays a normal fp32
        gamma, beta = gamma * 1e-37, beta * 1e-36
    elif kind == "huge":
        gamma, beta = gamma * 2e33, beta * 2e34       # bound 4e34 .. 1e36: above 2^114 = 2.1e34, far below fp32's maximum
    return dict(stats=stats, gamma=gamma.float(), beta=beta.float(), mmean=mmean.float(), mvar=mvar.float(),
                inv_count=1.0 / AFF_COUNT, C=C, groups=groups, p_gstride=C if p_gstride else 0)


def aff_ref(F, mode, dsc, inv_count=None, once=False, reverse=False):
    """``aff_kernel`` in float64 -> dict: ``s``, ``t`` (groups, C) and allowances ``a_s``, ``a_t``; ``mm``, ``mv``
    (the moving statistics after the call) with ``a_mm``, ``a_mv``; ``q`` (groups, C), the slot sums of squares.
    ``inv_count`` (the float normaliser), ``once`` (repeat ignored) and ``reverse`` (groups updated last to first)
    are the mutations of the CPU tests."""
    M = aff_mode(mode)
    C, groups, pgs = F["C"], F["groups"], F["p_gstride"]
    ic = F["inv_count"] if inv_count is None else inv_count
    gamma, beta, mm, mv = (G.f64(F[k]).clone() for k in ("gamma", "beta", "mmean", "mvar"))
    a_mm, a_mv = torch.zeros_like(mm), torch.zeros_like(mv)
    s, t, a_s, a_t = (torch.zeros(groups, C, dtype=torch.float64) for _ in range(4))
    batch = []
    for g in range(groups):
        po = g if pgs else 0
        if M["stats"]:
            batch.append(G.bn_moments64(F["stats"][g], ic))
        if M["stats"] and not M["running"]:
            mean, var, eu2 = batch[g]
            vrel = 0.5 * 2.0 ** -50 * eu2 / (var + EPS)
        else:
            mean, var, vrel = mm[po], mv[po], 0.0
        sc = gamma[po] / torch.sqrt(var + EPS)
        s[g], t[g] = sc * dsc, (beta[po] - mean * sc) * dsc
        a_s[g] = (2.0 ** -21 + vrel) * s[g].abs() + TINY
        a_t[g] = (2.0 ** -21 * (beta[po].abs() + (mean * sc).abs()) + vrel * (mean * sc).abs()) * dsc + 2 * TINY
    if M["update"]:
        om = 1.0 - MOMENTUM
        for g in (reversed(range(groups)) if reverse else range(groups)):
            po = g if pgs else 0
            mean, var, eu2 = batch[g]
            for _ in range(1 if once else M["repeat"]):
                a_mm[po] = a_mm[po] * MOMENTUM + 2.0 ** -22 * ((mm[po] * MOMENTUM).abs() + (mean * om).abs()) \
                    + om * 2.0 ** -23 * mean.abs()
                a_mv[po] = a_mv[po] * MOMENTUM + 2.0 ** -22 * ((mv[po] * MOMENTUM).abs() + var * om) \
                    + om * (2.0 ** -23 * var + 2.0 ** -50 * eu2)
                mm[po] = mm[po] * MOMENTUM + mean * om
                mv[po] = mv[po] * MOMENTUM + var * om
    q = F["stats"][:, :, 1].sum(1) if M["stats"] else None
    return dict(s=s, t=t, a_s=a_s, a_t=a_t, mm=mm, mv=mv, a_mm=a_mm, a_mv=a_mv, q=q)


def gscale_bound(s, t, q):
    """(groups,) float64: max_c(|s_c| sqrt(q_c) 1.0001 + |t_c|), the bound ``aff_kernel`` takes its exponent from."""
    return (s.abs() * torch.sqrt(q.clamp_min(0.0)) * 1.0001 + t.abs()).amax(1)


def amax_of(aff):
    """(groups, 2) fp32: max_c |aff| of each row of (groups, 2, C) -- what ``x3_aff`` writes beside the affine."""
    return aff.float().abs().amax(2)


# ------------------------------------------------------------------------------------------ layers, per sample
PS_LAYERS = [1, 2, 3, 4, 5]
PS_NWIN = [1, 11]
PS_CASES = [(l, n, v) for l in PS_LAYERS for n in PS_NWIN for v in ("hash_shared", "sign", "plain")
            if v != "hash_shared" or l == 1]
TILE_S = {1: 4, 2: 2, 3: 4, 4: 2, 5: 4}    # samples per tile (csrc/x3_geo.h layer table)


def window_exps(n_win, exps=SCALE_EXPS):
    return torch.tensor([exps[i % len(exps)] for i in range(n_win)], dtype=torch.int64)


def scale_windows(c, exps):
    """Window i of every group times 2^exps[i] (exact; signs and -0 kept), and ``smax_in`` from the scaled data."""
    c = dict(c)
    reps = c["r_in"].shape[0] // c["n_win"]
    f = torch.pow(2.0, exps.repeat(reps).double()).float()[:, None, None]
    c["r_in"] = c["r_in"] * f
    c["smax_in"] = f32_bits(c["r_in"].abs().amax((1, 2)))
    return c


def ps_case(l, n_win, variant, exps=None, zero_shift=False, zero_bias=False):
    """One per-sample-prescale ``x3_layer`` call: the rowdesc file's case with its folded group prescale taken
    out again (exact), ``amax`` as ``x3_aff`` writes it for this affine, the windows scaled by 2^exps (default:
    ``SCALE_EXPS`` cycling) and ``smax_in`` the bits of each input sample's max |R|."""
    c = dict(RD._case(l, n_win, variant))
    aff = (c["aff"] * c["gscale"]).float()        # 2^10 2^-10: exact
    if zero_shift:
        aff[:, 1] = 0.0
    c["aff"], c["gscale"] = aff, None
    if zero_bias:
        c["bias"] = torch.zeros_like(c["bias"])
    c["amax"] = amax_of(aff)
    c["variant"] = variant
    return scale_windows(c, window_exps(n_win) if exps is None else exps)


def slice_case(c, a):
    """Windows [a:] of every group as a case of their own (launched with ``window_offset + a``)."""
    n = c["n_win"]
    d = dict(c)
    reps = c["r_in"].shape[0] // n
    d["r_in"] = c["r_in"].view(reps, n, L, -1)[:, a:].reshape(reps * (n - a), L, -1).contiguous()
    d["smax_in"] = c["smax_in"].view(reps, n)[:, a:].reshape(-1).contiguous()
    d["n_win"] = n - a
    return d


def neighbour(sa):
    """The exponent of the other slot of the sample's slot pair (a tile starts at a multiple of its 2 or 4
    samples); a slot past the last window holds exponent 0."""
    idx = torch.arange(sa.shape[0]) ^ 1
    return torch.where(idx < sa.shape[0], sa[idx.clamp_max(sa.shape[0] - 1)], torch.zeros_like(sa))


def layer_ref(v, aff, keep, fr, wscale, bias, k, cin, cout, sa=None, sa_epi=None, conv=None):
    """One group of one layer in float64, (n, 60, cout): the staging's fp32 fma where ``keep``, times 2^sa per
    sample before the fp16 split, the split product (``x3.emulate_conv``) times 2^-sa_epi, bias, ReLU."""
    h = torch.where(keep, (v.double() * aff[0].double() + aff[1].double()).float(), torch.zeros(()))
    if sa is not None:
        h = h * torch.pow(2.0, sa.double()).float()[:, None, None]
        sa_epi = sa if sa_epi is None else sa_epi
    y = (conv or x3.emulate_conv)(h, fr, wscale, k, cin, cout)
    if sa is not None:
        y = y * torch.pow(2.0, -sa_epi.double())[:, None, None]
    return (y + bias.double()).clamp_min(0.0)


def ps_keep(c, g, channels_of="in", win_off=WIN_OFF, layer_shift=0, pass_shift=0):
    """Group g's keep mask of the input (the stream of block l - 1) or the output (block l) from ``ops/rng.py``."""
    l, n = c["l"], c["n_win"]
    if channels_of == "in":
        layer, ch, rate = l - 1, c["cin"], c["rate_in"]
    else:
        layer, ch, rate = l, c["cout"], c["rate_out"]
    key = rng.stream_key(SEED, layer + layer_shift, PASS_BASE + g + pass_shift)
    return G.keep_mask(key, win_off, n, L, ch, rate)


def ps_exponents(c, g, smax=None):
    """-> (sa (n,), the float64 bounds) of group g's samples."""
    n = c["n_win"]
    sm = c["smax_in"] if smax is None else smax
    sm = sm if c["shared"] else sm[g * n:(g + 1) * n]
    return sample_prescale_ref(c["amax"][0 if c["shared"] else g], bits_f32(sm))


def layer_ps_ref(c, win_off=WIN_OFF, stage=None, epi=None, smax=None, layer_shift=0, pass_shift=0, conv=None):
    """float64 R_l of every group, (GROUPS, n_win, 60, cout), as the PS kernel forms it: ``_emulate`` of the
    rowdesc file with each sample's staged h times 2^sa before ``split_f16`` and the product times 2^-sa.
    Mutations (CPU tests): ``stage`` / ``epi`` map the exponents used in staging / in the epilogue, ``smax``
    replaces the per-sample maxima, ``layer_shift`` / ``pass_shift`` move the input mask's stream, ``conv``
    replaces the split product."""
    n, cin, cout, k = c["n_win"], c["cin"], c["cout"], c["k"]
    outs = []
    for g in range(GROUPS):
        v = c["r_in"] if c["shared"] else c["r_in"][g * n:(g + 1) * n]
        if c["sign_in"]:
            keep = ~torch.signbit(v)
        elif c["rate_in"]:
            keep = ps_keep(c, g, "in", win_off, layer_shift, pass_shift)
        else:
            keep = torch.ones_like(v, dtype=torch.bool)
        sa = ps_exponents(c, g, smax)[0]
        gw = g if c["per_group"] else 0
        outs.append(layer_ref(v, c["aff"][0 if c["shared"] else g], keep, c["frs"][gw], c["scs"][gw], c["bias"][gw], k,
                              cin, cout, sa if stage is None else stage(sa), sa if epi is None else epi(sa), conv))
    return torch.stack(outs)


def per_sample_rel(got, want):
    """(groups, n): max |got - want| over the sample / max |want| of the sample (a non-finite entry counts as inf)."""
    got, want = got.double().flatten(2), want.double().flatten(2)
    d = (got - want).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return d.amax(2) / want.abs().amax(2)


def block6_sums(want, keep):
    """S1 = sum_t keep R, S0 = sum_t keep of (groups, n, 60, C)."""
    return (want * keep).sum(2), keep.sum(2).float()


# ------------------------------------------------------------------------------------------ head
HEAD_SHAPES = [(1, 1), (3, 1), (5, 1), (2, 3), (7, 2)]     # (n_win, groups)
HEAD_BIASES = [0.25, 30.0, -30.0, 100.0, -100.0]
HEAD_C = x3.CH[6]


def head_fixture(n_win, groups, per_aff, per_dense, bias):
    """sums (samples, 2, C): S1 >= 0 and S0 the integer keep counts block 6 writes; affine (groups or 1, 2, C) and
    dense weights / bias (groups or 1), distinct per group."""
    gen = G._gen(33, n_win, groups, per_aff, per_dense, int(bias * 4))
    C, n = HEAD_C, n_win * groups
    s0 = (torch.rand(n, L, C, generator=gen) >= 0.2).sum(1).float()
    s1 = 1.5 * torch.rand(n, C, generator=gen) * s0
    ga, gp = (groups if per_aff else 1), (groups if per_dense else 1)
    aff = torch.stack([1.25 * (0.5 + torch.rand(ga, C, generator=gen)), 0.3 * torch.randn(ga, C, generator=gen)], 1)
    dw = torch.randn(gp, C, generator=gen) / math.sqrt(C)
    db = bias + 0.125 * torch.arange(gp)
    return dict(sums=torch.stack([s1, s0], 1).float(), aff=aff.float(), dw=dw.float(), db=db.float(), n_win=n_win,
                groups=groups, aff_gstride=2 * C if per_aff else 0, p_gstride=C if per_dense else 0)


def head_ref(F, inv=1.0 / L, aff_group0=False, dense_group0=False):
    """``head_kernel`` in float64 -> (logit, its allowance, probability, its allowance), each (samples,).

    The kernel's plain ``1 / (1 + expf(-z))`` returns 0 where the true probability is subnormal (expf overflows
    or the quotient is flushed): that is within the 2^-126 absolute term and not a defect.  ``inv`` and the
    ``*_group0`` flags are the mutations of the CPU tests."""
    sums, aff, dw, db = (G.f64(F[k]) for k in ("sums", "aff", "dw", "db"))
    n, C = sums.shape[0], sums.shape[2]
    g = torch.arange(n) // F["n_win"]
    ga = g if F["aff_gstride"] and not aff_group0 else torch.zeros_like(g)
    gp = g if F["p_gstride"] and not dense_group0 else torch.zeros_like(g)
    a, b = aff[ga, 0] * sums[:, 0], aff[ga, 1] * sums[:, 1]
    z = (dw[gp] * (a + b)).sum(1) * inv + db[gp]
    terms = (dw[gp].abs() * (a.abs() + b.abs())).sum(1) / L
    a_z = (2 * -(-C // 64) + 6 + 4) * U32 * terms + U32 * db[gp].abs()
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    return z, a_z, p, a_z * p * q + 4 * U32 * p + 2.0 ** -126
