"""References of the batch-moment ``layer_kernel`` instances of ``csrc/x3_layers.hip`` (blocks 2..6, slot and
dense-row mappings) in three levels, the per-entry allowances between them, exact-arithmetic probes and the
fixtures both test files share (``test_x3_layer_refs_cpu.py`` checks this oracle without a GPU,
``test_x3_layer_kernels_gpu.py`` holds the kernels to it).  The probes also serve the ``PS = true`` kernels.

(a) THE SPLIT (:func:`stage`): the staging's fp32 ``fma(v, s, t)`` of the kernel's own fp32 inputs, masked, then
    the fp16 halves ``hi = fp16(a)``, ``lo = fp16(a - hi)``.
(b) THE MODEL (:func:`model`): in float64 the sum ``hi hi + lo hi + hi lo`` over the packed weight fragments,
    times ``wscale[g] gscale[g]`` (one fp32 factor, exact powers of two), plus the bias, then ReLU.  What is left
    between a kernel and its model is fp32 accumulation alone.
(c) Plain float64 TRUTH (:func:`truth`): the conv of the un-prescaled staged activations with the fp32 kernel that
    ``x3.pack_conv`` was given.

Allowances (``U32 = 2^-23`` per fp32 operation, ``tests/generic_kernel_refs.py``):

* kernel against model, ``a1``: three MFMAs per k-step, each of the K = k Cin products counted as an addition, the
  epilogue's fma and slack: ``(3 K + 2) U32 (sum of the absolute terms + |b|)``.
* model against truth, ``a2``: the derivation of ``gx3_kernel_refs.truth_allow`` at this launcher's prescales.  A
  staged value ``a 2^sa`` and a weight ``w 2^sw`` are each hi + lo + r with ``|r| <= max(2^-22 |.|, 2^-25)``, and
  the lo lo product is dropped: three terms of ``2^-22 |a w|`` plus the floors ``2^-25 2^-sa |w|`` and
  ``2^-25 2^-sw |a|`` and ``2^-50 2^-(sa + sw)`` where both meet, times 1.01 for the second-order products.
  ``2^-sa`` is the group's ``gscale`` and ``2^-sw`` the layer's (member's) ``wscale``.
* signs, mask zeros and ``S0`` are exact.  Block 6's ``S1``: the entries' allowances summed over the kept steps
  plus 60 fp32 additions over the kept sum.
* moments: a lane adds its row tiles and 16 lanes are summed, all within one tile, in fp32; tiles and slots are
  fp64: ``(tile rows + tiles per slot + 2) U32 sum`` against float64 sums of the stored outputs (every term is
  >= 0).  Block 6 stores no R_6: the model's sums, with the entries' allowances carried into both moments.

Probes (tier 2): activations and kernels of ``gx3_kernel_refs`` (``probe_acts``, ``probe_nets``): a staged value
is +-(H + j 2^-13) 2^e with H = 1..15 on the fp16 grid, so ``hi = H``, ``lo = j 2^-13`` at every prescale that
keeps lo normal; kernels hold +-1, +-2, +-(1 + 2^-12).  Every product without lo lo is a multiple of 2^-13 and the
absolute terms of an entry sum below 2^11: exact in fp32 in any order (:func:`probe_exact`).  The epilogue's one
fma is one rounding of an exact float64 value, so ``model(...).float()`` is the kernel's output bit for bit.
"""
import re
from pathlib import Path

import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng, x3

from . import generic_kernel_refs as G
from . import gx3_kernel_refs as G3
from . import x3_kernel_refs as X

U32 = G.U32
L = X.L
GROUPS = 3
SEED, PASS_BASE, WIN_OFF = X.SEED, X.PASS_BASE, X.WIN_OFF
GRID = X.GRID
GRIDS = [1, 7, 1000]                  # compared with GRID = 3; 1000: no smaller than any case's tile count (the launcher
                                      # clamps it to that: one tile per workgroup)
GROUP_EXPS = (10, 3, -6)              # group g's affine is prescaled by 2^GROUP_EXPS[g], its gscale is 2^-that
PROBE_EXPS = (10, 3, -1)              # the probes keep lo = j 2^-13 2^e a normal fp16
EQUI_J = (1, -4, -2)                  # group equivariance: affine times 2^j, gscale times 2^-j
WFAC = (1.0, 1.3 * 2.0 ** -5, 0.7 * 2.0 ** 4)   # per-member kernels of different magnitude: wscale differs
PROBE_WEXP = (0, -3, 2)               # the probe nets of the three members times 2^that
SMALL = 2.0 ** -12
RATE_IN, RATE_OUT = X.RD.RATE_IN, X.RD.RATE_OUT
SIGN_LAYERS = X.RD.SIGN_LAYERS
LAYERS = [1, 2, 3, 4, 5]
VARIANTS = ["hash", "sign", "plain", "shared"]
TILE_S = X.TILE_S                     # samples per tile, csrc/x3_geo.h (held to the header by the CPU tests)
SLOTS = X.SLOTS


# ================================================================================================ geometry
def layer_table():
    """{layer: (cin, cout, k, S, dense)} read from the committed table of ``csrc/x3_geo.h``."""
    src = Path(x3.__file__).resolve().parents[1] / "csrc" / "x3_geo.h"
    text = src.read_text().split("#define APNEAUQ_X3_LAYERS(X)")[1].split("#endif")[0]
    rows = re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\w+), (-?\d+), (-?\d+), (\d+), (\d+), (\w+)\)", text)
    return {int(r[0]): (int(r[1]), int(r[2]), int(r[3]), int(r[4]), r[12] == "true" and r[7] == "false") for r in rows}


def tile_rows(l):
    return 64 * TILE_S[l]


def tiles_per_group(dense, n_win, S):
    """``x3_geo.h:tiles_per_group``."""
    return -(-L * n_win // (64 * S)) if dense else -(-n_win // S)


def tile_geo(dense, S, tile, tpg, n_win):
    """``x3_geo.h:tile_geo`` -> dict(g, w0, wf, off, rows_left); rows_left unclamped."""
    g = tile // tpg
    w0 = (tile - g * tpg) * (64 * S if dense else S)
    wf = w0 // L if dense else w0
    off = w0 - wf * L if dense else 0
    return dict(g=g, w0=w0, wf=wf, off=off, rows_left=(n_win - wf) * L - off)


def tiles_per_slot(dense, l, n_win, groups, grid):
    """The most tiles of one group that any moment slot (workgroup % 16) receives."""
    tpg = tiles_per_group(dense, n_win, TILE_S[l])
    total = tpg * groups
    grid = min(grid, total)
    count = {}
    for wg in range(grid):
        for t in range(wg * total // grid, (wg + 1) * total // grid):
            key = (t // tpg, wg % SLOTS)
            count[key] = count.get(key, 0) + 1
    return max(count.values())


def nwin_cases(l):
    """The window counts of layer l: below and across a slot tile; then the dense tile edges of its tile size."""
    return [1, 2, 3, 5] + ([15, 32] if tile_rows(l) == 128 else [47, 64])


def tier1_cases():
    """(l, n_win, variant): every layer meets every n_win once, the variants in rotation."""
    return [(l, n, VARIANTS[(i + l) % 4]) for l in LAYERS for i, n in enumerate(nwin_cases(l))]


# ================================================================================================ masks
def keep_mask(layer, g, n_win, channels, thr, layer_shift=0, same_pass=False, win_off=WIN_OFF, swap=False,
              pass_base=PASS_BASE):
    """``ops/rng.py`` keep mask of group g's windows (n_win, 60, channels) at a 16-bit threshold.  Mutations (CPU
    tests): the stream of another layer, pass_base for pass_base + g, window_offset dropped, the 16-bit halves
    of a hash swapped (channels c and c ^ 1 exchanged)."""
    key = rng.stream_key(SEED, layer + layer_shift, pass_base + (0 if same_pass else g))
    keep = rng.keep_mask_torch(key, win_off + torch.arange(n_win), L, channels, thr / 65536.0)
    return keep[:, :, torch.arange(channels) ^ 1] if swap else keep


def in_keep(c, g, **mut):
    v = group_in(c, g)
    if c["sign_in"] and c["thr_in"]:
        return ~torch.signbit(v)
    if c["thr_in"]:
        return keep_mask(c["l"] - 1, g, c["n_win"], c["cin"], c["thr_in"], **mut)
    return torch.ones_like(v, dtype=torch.bool)


def out_keep(c, **mut):
    """(GROUPS, n_win, 60, cout): block l's mask where this call draws it (sign_out, or block 6), else all kept."""
    if c["thr_out"] and (c["sign_out"] or c["l"] == 5):
        return torch.stack([keep_mask(c["l"], g, c["n_win"], c["cout"], c["thr_out"], **mut) for g in range(GROUPS)])
    return torch.ones(GROUPS, c["n_win"], L, c["cout"], dtype=torch.bool)


# ================================================================================================ fixtures
def _masks(c, l, variant, gen):
    """thr_in / thr_out / sign_in / sign_out of a variant; the sign variant's input carries its mask."""
    c.update(sign_in=False, sign_out=False, thr_in=0, thr_out=0)
    if variant in ("hash", "shared"):
        c.update(thr_in=rng.dropout_threshold(RATE_IN), thr_out=rng.dropout_threshold(RATE_OUT) if l == 5 else 0)
    elif variant == "sign":
        si, so = x3._sign(l, SIGN_LAYERS)
        c.update(sign_in=si, sign_out=so, thr_in=rng.dropout_threshold(RATE_IN), thr_out=rng.dropout_threshold(RATE_OUT))
        if si:   # the producer's mask travels in the sign bit (a dropped zero is -0)
            r = c["r_in"]
            r = torch.where(torch.rand(r.shape, generator=gen) < RATE_IN, -r, r)
            r[0, :, 0] = -0.0
            c["r_in"] = r


def case(l, n_win, variant, equivariant=False):
    """One batch-moment ``x3_layer`` call on 3 groups.

    * group g's affine is prescaled by 2^GROUP_EXPS[g] and its ``gscale`` is 2^-GROUP_EXPS[g]; every prescaled
      affine has the magnitude 2^10, so the un-prescaled activations of the groups lie 2^7 apart;
    * every member has its own kernel, bias and ``wscale`` (``WFAC``) -- but ``variant = "shared"``: one input, one
      affine, one kernel for all groups (the strides of 0, block 2 under MC Dropout);
    * input channels c % 8 == 1 have a negative scale, c % 8 == 6 a scale of zero, c % 8 == 3 scale and shift at
      2^-12 of the others'; output channels co % 16 == 7 have kernel and bias at 2^-12 of the others': small
      staged values and small output entries in every tile, beside the largest;
    * ``equivariant``: shift and scale of a channel have one sign, |shift| >= 0.05, nothing small, prescale 2^9:
      every non-zero staged value lies in [2^4, 2^13.5), so EQUI_J keeps it inside [2^-3, 2^14)."""
    cin, cout, k = x3.CH[l], x3.CH[l + 1], x3.KS[l]
    gen = G._gen(41, l, n_win, VARIANTS.index(variant), int(equivariant))
    shared = variant == "shared"
    ng = 1 if shared else GROUPS
    c = dict(l=l, n_win=n_win, cin=cin, cout=cout, k=k, variant=variant, shared=shared, per_group=not shared)
    c["r_in"] = torch.randn(n_win * ng, L, cin, generator=gen).abs().float()
    _masks(c, l, variant, gen)
    ci, co = torch.arange(cin), torch.arange(cout)
    s = 0.5 + torch.rand(ng, cin, generator=gen)
    t = 0.3 * torch.randn(ng, cin, generator=gen)
    s[:, ci % 8 == 1] *= -1.0
    s[:, ci % 8 == 6] = 0.0
    if equivariant:
        t = torch.where(s < 0, -1.0, 1.0) * (0.05 + t.abs())
    else:
        s[:, ci % 8 == 3] *= SMALL
        t[:, ci % 8 == 3] *= SMALL
    base = 9 if equivariant else 10
    c["aff"] = (torch.stack([s, t], 1) * 2.0 ** base).float()                     # (ng, 2, cin), prescaled
    c["gscale"] = torch.tensor([2.0 ** -e for e in GROUP_EXPS[:ng]], dtype=torch.float32)
    mag = [2.0 ** (base - e) for e in GROUP_EXPS[:ng]]                            # of the un-prescaled activations
    ws, bs = [], []
    for g in range(ng):
        w = 0.05 * WFAC[g] * torch.randn(k, cin, cout, generator=gen)
        b = 0.1 * WFAC[g] * mag[g] * torch.randn(cout, generator=gen)
        w[:, :, co % 16 == 7] *= SMALL
        b[co % 16 == 7] *= SMALL
        ws.append(w.float())
        bs.append(b.float())
    return _pack(c, ws, bs)


def _pack(c, ws, bs):
    c["w"], c["bias"] = ws, torch.stack(bs).float()
    frs, scs = zip(*[x3.pack_conv(w) for w in ws])
    c["frs"], c["scs"] = list(frs), list(scs)
    return c


def rescale_groups(c, js):
    """Group g's affine times 2^js[g] and its gscale times 2^-js[g] (exact)."""
    d = dict(c)
    f = torch.tensor([2.0 ** j for j in js[:c["aff"].shape[0]]], dtype=torch.float32)
    d["aff"] = c["aff"] * f[:, None, None]
    d["gscale"] = c["gscale"] / f
    return d


def staged_range(c):
    """(smallest non-zero, largest) |staged value| of a case, masks ignored."""
    lo, hi = float("inf"), 0.0
    for g in range(GROUPS):
        h = stage(group_in(c, g), c["aff"][ga(c, g)], torch.ones(c["n_win"], L, c["cin"], dtype=torch.bool))[0].abs()
        lo, hi = min(lo, float(h[h > 0].min())), max(hi, float(h.max()))
    return lo, hi


def ga(c, g):
    return g if c["aff"].shape[0] > 1 else 0


def gw(c, g):
    return g if len(c["frs"]) > 1 else 0


def group_in(c, g):
    n = c["n_win"]
    return c["r_in"] if c["shared"] else c["r_in"][g * n:(g + 1) * n]


# ---- the kernels' own chain: x3_aff(gscale) on per-group moment slots
AFF_CHAIN_MAG = (0, 8, -8)


def aff_chain_case(l, n_win):
    """Inputs whose groups lie 2^+-8 apart -- group 1 with a small relative spread (its bound is far above its
    values), group 2 below the BN epsilon -- their moment slots as block l's epilogue would leave them, and the BN
    parameters ``x3_aff`` turns into the affine and ``gscale`` of this call."""
    c = case(l, n_win, "hash")
    gen = G._gen(42, l, n_win)
    cin = c["cin"]
    r = c["r_in"].view(GROUPS, n_win, L, cin).clone()
    r[1] = 2.0 ** 8 * (1.0 + 2.0 ** -5 * r[1])
    r[2] = 2.0 ** -8 * r[2]
    c["r_in"] = r.view(-1, L, cin).contiguous()
    st = torch.zeros(GROUPS, SLOTS, 2, cin, dtype=torch.float64)
    for g in range(GROUPS):
        u = r[g].double().reshape(-1, cin)
        half = u.shape[0] // 2
        for slot, part in ((3 + g, u[:half]), (11, u[half:])):
            st[g, slot, 0] += part.sum(0)
            st[g, slot, 1] += (part * part).sum(0)
    gamma = 0.5 + torch.rand(1, cin, generator=gen)
    gamma[0, torch.arange(cin) % 8 == 1] *= -1.0
    gamma[0, torch.arange(cin) % 8 == 6] = 0.0
    c["bn"] = dict(stats=st, gamma=gamma.float(), beta=(0.3 * torch.randn(1, cin, generator=gen)).float(),
                   mmean=torch.zeros(1, cin), mvar=torch.ones(1, cin), inv_count=1.0 / (n_win * L), C=cin,
                   groups=GROUPS, p_gstride=0)
    return c


def aff_chain_expected(c):
    """What ``x3_aff(gscale=True)`` writes for :func:`aff_chain_case`, from ``x3_kernel_refs.aff_ref``:
    (aff (GROUPS, 2, cin) float64 prescaled, the exponents sa (GROUPS,), the bounds)."""
    A = X.aff_ref(c["bn"], "batch_gscale", X.DSC)
    bnd = X.gscale_bound(A["s"], A["t"], A["q"])
    sa = X.prescale_exp(bnd)
    f = torch.pow(2.0, sa.double())[:, None]
    return torch.stack([A["s"] * f, A["t"] * f], 1), sa, bnd


# ================================================================================================ level (a)
def stage(v, aff, keep, sa=None):
    """The staged activations of one group: (a fp32, hi, lo as float64).  ``sa`` (n,): the per-sample exponents of
    the PS kernels (``ldexpf`` after the fma)."""
    a = torch.where(keep, (v.double() * aff[0].double() + aff[1].double()).float(), torch.zeros(()))
    if sa is not None:
        a = a * torch.pow(2.0, sa.double()).float()[:, None, None]
    hi = a.half()
    lo = (a - hi.float()).half()
    return a, hi.double(), lo.double()


def frag_halves(fr, k, cin, cout):
    """The packed fragments as two float64 kernels (k, cin, cout): hi and lo of w 2^sw."""
    v = fr.reshape(cin // x3.CK, k, cout // 16, 2, 4, 16, 8).double()
    return tuple(v[:, :, :, i].permute(1, 0, 3, 5, 2, 4).reshape(k, cin, cout) for i in (0, 1))


# ================================================================================================ level (b)
def _pad(x, p, mode=None, nxt=None):
    """(n, 60, C) -> (n, 60 + 2 p, C) with the conv's zero halo.  Mutations: ``"neighbour"`` -- the halo rows are
    the neighbouring windows' rows; ``"past_end"`` -- the rows after the group's last window are ``nxt``'s."""
    n, _, C = x.shape
    xp = torch.zeros(n, L + 2 * p, C, dtype=x.dtype)
    xp[:, p:p + L] = x
    if mode == "neighbour" and n > 1:
        xp[1:, :p] = x[:-1, L - p:]
        xp[:-1, p + L:] = x[1:, :p]
    if mode == "past_end" and nxt is not None:
        xp[-1, p + L:] = nxt[:p]
    return xp


def _conv(xp, w):
    """'valid' float64 conv of padded windows (n, 60 + 2 p, cin) with (k, cin, cout)."""
    return torch.nn.functional.conv1d(xp.permute(0, 2, 1), w.permute(2, 1, 0)).permute(0, 2, 1)


def split_product(ah, al, whi, wlo, drop=(), mode=None, nxt=(None, None)):
    """(sum, sum of the absolute terms) of hi hi + lo hi + hi lo, (n, 60, cout).  ``drop``: "lo_hi" (w.lo a.hi) /
    "hi_lo" (w.hi a.lo) left out; ``mode``: :func:`_pad`'s mutations, or ``"tap_shift"`` -- the first row of every
    window reads every tap one row further down."""
    p = (whi.shape[0] - 1) // 2
    wa = whi if "lo_hi" in drop else whi + wlo          # exact in float64
    wab = whi.abs() if "lo_hi" in drop else whi.abs() + wlo.abs()
    pad = mode if mode in ("neighbour", "past_end") else None
    hp, lp = _pad(ah, p, pad, nxt[0]), _pad(al, p, pad, nxt[1])
    y, ab = _conv(hp, wa), _conv(hp.abs(), wab)
    if "hi_lo" not in drop:
        y, ab = y + _conv(lp, whi), ab + _conv(lp.abs(), whi.abs())
    if mode == "tap_shift":
        z = torch.zeros_like(hp[:, :1])
        ys = _conv(torch.cat([hp[:, 1:], z], 1), wa) + _conv(torch.cat([lp[:, 1:], z], 1), whi)
        y = y.clone()
        y[:, 0] = ys[:, 0]
    return y, ab


def model(c, drop=(), mode=None, gscale_of=None, aff_of=None, wscale_of=None, mask=None, sa=None, sa_epi=None):
    """Level (b) of every group -> dict: ``y`` (GROUPS, n, 60, cout) float64 after the ReLU; ``core`` / ``ab``:
    the product times the epilogue factor before the bias, and its absolute terms with |b|; ``a1``: the
    kernel-against-model allowance; ``h``: the staged fp32 values per group; ``keep``: the input masks.
    ``*_of``: group index maps (the group-0 mutations); ``mask``: :func:`keep_mask` mutations of the input mask;
    ``sa`` (GROUPS, n): per-sample exponents (PS), ``sa_epi`` those undone in the epilogue."""
    l, n, cin, cout, k = c["l"], c["n_win"], c["cin"], c["cout"], c["k"]
    ident = lambda g: g
    gscale_of, aff_of, wscale_of = gscale_of or ident, aff_of or ident, wscale_of or ident
    st = []
    for g in range(GROUPS):
        keep = in_keep(c, g, **(mask or {}))
        st.append(stage(group_in(c, g), c["aff"][ga(c, aff_of(g))], keep, None if sa is None else sa[g]) + (keep,))
    ys, cores, abs_ = [], [], []
    for g in range(GROUPS):
        whi, wlo = frag_halves(c["frs"][gw(c, g)], k, cin, cout)
        nx = st[(g + 1) % GROUPS]
        y, ab = split_product(st[g][1], st[g][2], whi, wlo, drop, mode, (nx[1][0], nx[2][0]) if g + 1 < GROUPS else (None, None))
        f = float(torch.tensor(c["scs"][gw(c, wscale_of(g))], dtype=torch.float32))
        if c.get("gscale") is not None:
            f = f * float(c["gscale"][ga(c, gscale_of(g))])
        f = torch.full((n, 1, 1), f, dtype=torch.float64)
        if sa is not None:
            f = f * torch.pow(2.0, -(sa if sa_epi is None else sa_epi)[g].double())[:, None, None]
        b = c["bias"][gw(c, g)].double()
        cores.append(y * f)
        abs_.append(ab * f + b.abs())
        ys.append((y * f + b).clamp_min(0.0))
    ab = torch.stack(abs_)
    return dict(y=torch.stack(ys), core=torch.stack(cores), ab=ab, a1=(3 * k * cin + 2) * U32 * ab,
                h=[s[0] for s in st], keep=[s[3] for s in st])


# ================================================================================================ level (c)
def truth(c, M):
    """Plain float64 of the un-prescaled staged activations (``M = model(c)``; masked, fp32 as the kernel forms
    them) and the fp32 kernels -> (R (GROUPS, n, 60, cout), the model-against-truth allowance)."""
    k, cin, cout, n = c["k"], c["cin"], c["cout"], c["n_win"]
    one_x = torch.ones(1, L, cin, dtype=torch.float64)
    ys, als = [], []
    for g in range(GROUPS):
        fa = float(c["gscale"][ga(c, g)])                   # 2^-sa
        fw = c["scs"][gw(c, g)]                             # 2^-sw
        a = M["h"][g].double() * fa
        w = c["w"][gw(c, g)].double()
        ys.append((G.conv64(a, w) + c["bias"][gw(c, g)].double()).clamp_min(0.0))
        prod = G.conv_abs64(a, w)
        sum_w = G.conv64(one_x, w.abs())                    # over the taps inside the sample
        sum_x = G.conv64(a.abs(), torch.ones(k, cin, 1, dtype=torch.float64))
        cnt = G.conv64(one_x, torch.ones(k, cin, 1, dtype=torch.float64))
        als.append(G3.SLACK * (3 * G3.SPLIT_REL * prod + G3.SPLIT_FLOOR * (fa * sum_w + fw * sum_x)
                               + G3.SPLIT_FLOOR ** 2 * fa * fw * cnt))
    return torch.stack(ys), torch.stack(als)


_cache = {}


def refs(key, build):
    """Model, truth and allowances of one case, computed once and shared (read-only)."""
    if key not in _cache:
        c = build()
        M = model(c)
        T, a2 = truth(c, M)
        _cache[key] = dict(c=c, M=M, T=T, a2=a2)
    return _cache[key]


def tier1_refs(l, n_win, variant):
    return refs(("t1", l, n_win, variant), lambda: case(l, n_win, variant))


# ================================================================================================ sums and moments
def block6_sums(y, keep):
    """S1 = sum_t keep R, S0 = sum_t keep of (GROUPS, n, 60, C)."""
    return (y * keep).sum(2), keep.sum(2).float()


def s1_allow(y, a1, keep):
    return (a1 * keep).sum(2) + L * U32 * (y * keep).sum(2)


def moments(y):
    """(GROUPS, 2 C) float64: sum R, sum R^2 over a group's rows of (GROUPS, n, 60, C)."""
    r = y.double().abs()
    return torch.cat([r.sum((1, 2)), (r * r).sum((1, 2))], 1)


def moment_allow(msum, dense, l, n_win, grid):
    return (tile_rows(l) + tiles_per_slot(dense, l, n_win, GROUPS, grid) + 2) * U32 * msum


def model_moment_allow(y, a1):
    """What the entries' own allowances add to sums taken from the model (block 6 stores no R_6)."""
    return torch.cat([a1.sum((1, 2)), (2 * y * a1 + a1 * a1).sum((1, 2))], 1)


def past_end_rows(dense, l, n_win):
    """Accumulator rows of a group's last tile that lie past the group's end."""
    S = TILE_S[l]
    return tiles_per_group(dense, n_win, S) * (64 * S if dense else L * S) - L * n_win


# ================================================================================================ probes
PROBE_T = (0, 3, 7, 0, 5)     # |shift| of channel c: PROBE_T[c % 5]
PROBE_NWIN = 5
PROBE_PS_EXPS = X.SCALE_EXPS  # window i of a PS probe is scaled by 2^PROBE_PS_EXPS[i % 5]
PS_VARIANTS = ["sign", "plain", "shared"]        # of the PS probes, CPU and GPU file alike
MOMENT_VARIANTS = ["hash", "sign", "plain"]      # of the small-output probes
S1_CASES = [(v, ps) for ps in (False, True) for v in ("hash", "sign", "plain")]   # of block 6's S1 probe


def probe_case(l, n_win, variant, ps=False):
    """An exact-arithmetic call.  Inputs H' + j 2^-13 with H' = 1..8, j = 1..3 (``gx3_kernel_refs.probe_acts``),
    scales +-1 (c % 8 == 1: -1) and 0 (c % 8 == 6) and shifts of the scale's sign with |t| in PROBE_T, all times
    2^PROBE_EXPS[g]: a staged value is +-(H + j 2^-13) 2^e with H <= 15, or a bare shift.  Member g's kernel is
    ``gx3_kernel_refs.probe_nets``'s rolled by g output channels and scaled by 2^PROBE_WEXP[g]; integer biases of
    both signs.  ``ps``: no group prescale and no shift; window i times 2^PROBE_PS_EXPS[i % 5], ``smax_in`` and
    ``amax`` as block l and ``x3_aff`` leave them."""
    cin, cout, k = x3.CH[l], x3.CH[l + 1], x3.KS[l]
    shared = variant == "shared"
    ng = 1 if shared else GROUPS
    gen = G._gen(43, l, n_win, VARIANTS.index(variant), int(ps))
    c = dict(l=l, n_win=n_win, cin=cin, cout=cout, k=k, variant=variant, shared=shared, per_group=not shared, probe=True)
    r = G3.probe_acts(n_win * ng, L, cin, 7 * l + len(variant)).abs()
    c["r_in"] = torch.where(r >= 9.0, r - 8.0, r).float()
    exps = X.window_exps(n_win, PROBE_PS_EXPS) if ps else torch.zeros(n_win, dtype=torch.int64)
    c["win_exps"] = exps
    c["r_in"] = c["r_in"] * torch.pow(2.0, exps.repeat(ng).double()).float()[:, None, None]
    _masks(c, l, variant, gen)
    ci = torch.arange(cin)
    s = torch.ones(cin)
    s[ci % 8 == 1] = -1.0
    s[ci % 8 == 6] = 0.0
    t = torch.where(s < 0, -1.0, 1.0) * torch.tensor(PROBE_T, dtype=torch.float32)[ci % 5]
    if ps:
        t = torch.zeros(cin)
    f = torch.tensor([1.0] * ng if ps else [2.0 ** e for e in PROBE_EXPS[:ng]])
    c["aff"] = (torch.stack([s, t])[None] * f[:, None, None]).float()
    c["gscale"] = None if ps else (1.0 / f).float()
    if ps:
        c["amax"] = X.amax_of(c["aff"])
        c["smax_in"] = X.f32_bits(c["r_in"].abs().amax((1, 2)))
    net = G3.probe_nets(k, cin, cout, False)
    assert len(net) == 1
    ws = [torch.roll(net[0], g, 2) * 2.0 ** PROBE_WEXP[g] for g in range(ng)]
    bs = [torch.roll(G3.probe_bias(cout), 5 * g) for g in range(ng)]
    # the grid of an entry's terms: 2^-13, times the member's and (PS) the window's power of two
    c["unit"] = torch.tensor([[2.0 ** (-13 + PROBE_WEXP[g] + int(e)) for e in exps] for g in range(GROUPS if not shared else 1)],
                             dtype=torch.float64).expand(GROUPS, n_win)[:, :, None, None]
    return _pack(c, ws, bs)


def moment_probe_case(l, n_win, variant):
    """Small outputs: inputs 0..3 (lo = 0), scales +-1 and 0 without a shift, four weights of +-1 per output
    channel, biases -1, 0, 1: R <= 13, so every tile's sum R and sum R^2 is an integer below 2^24 and the moment
    sums, block 6's S1 and S0 are exact."""
    c = probe_case(l, n_win, variant)
    cin, cout, k = c["cin"], c["cout"], c["k"]
    gen = G._gen(44, l, n_win, VARIANTS.index(variant))
    ng = c["aff"].shape[0]
    r = torch.randint(0, 4, c["r_in"].shape, generator=gen).float()
    c["r_in"] = torch.where(torch.signbit(c["r_in"]), -r, r)          # the sign variant's mask stays
    c["aff"][:, 1] = 0.0
    K = k * cin
    m = -(-K // 4)
    idx, co = torch.meshgrid(torch.arange(K), torch.arange(cout), indexing="ij")
    ws = []
    for g in range(ng):
        on = (idx + 7 * co + g) % m == 0
        w = torch.where(on, torch.where(idx % 3 == 0, -1.0, 1.0), 0.0)
        ws.append(w.reshape(k, cin, cout).float().contiguous())
    bs = [((torch.arange(cout) + g) % 3 - 1).float() for g in range(ng)]
    c["unit"] = torch.ones(GROUPS, n_win, 1, 1, dtype=torch.float64)
    c["moment_probe"] = True
    return _pack(c, ws, bs)


def s1_probe_case(variant, ps=False):
    """Block 6's probe for the fp16 halves.  Block 6 stores no R_6, so what a test sees of a dropped ``lo hi`` or
    ``hi lo`` is S1 = sum_t keep R: here it is exact.  Activations as :func:`probe_case` (lo != 0), every member's
    kernel two weights per output channel out of +-1 and +-(1 + 2^-12) (a lo in the weights too), no member
    factor, biases -2..2 (PS: 0, so that R stays on the window's grid): R < 32.1, and a sample's 60 kept steps sum
    below 2^11 = 2^24 grid units, so every partial sum of S1 is exact in fp32 in any order."""
    c = probe_case(5, PROBE_NWIN, variant, ps)
    cin, cout, k = c["cin"], c["cout"], c["k"]
    ng = c["aff"].shape[0]
    K = k * cin
    m = -(-K // 2)
    idx, co = torch.meshgrid(torch.arange(K), torch.arange(cout), indexing="ij")
    vals = torch.tensor([1.0, 1.0 + 2.0 ** -12, -1.0, -(1.0 + 2.0 ** -12)])[(idx // m + co) % 4]
    ws = [torch.where((idx + 7 * co + g) % m == 0, vals, torch.zeros(())).reshape(k, cin, cout).float().contiguous()
          for g in range(ng)]
    bs = [torch.zeros(cout) if ps else ((torch.arange(cout) + g) % 5 - 2).float() for g in range(ng)]
    c["unit"] = (2.0 ** -13 * torch.pow(2.0, c["win_exps"].double())).expand(GROUPS, PROBE_NWIN)[:, :, None, None]
    return _pack(c, ws, bs)


def s1_probe_refs(variant, ps):
    key = ("s1", variant, ps)
    if key not in _cache:
        c = s1_probe_case(variant, ps)
        _cache[key] = dict(c=c, M=probe_model(c))
    return _cache[key]


def s1_units(c, y, keep=None):
    """S1 of (GROUPS, n, 60, C) in the grid units of its sample, (GROUPS, n, C)."""
    return block6_sums(y, out_keep(c) if keep is None else keep)[0] / c["unit"][:, :, 0]


def probe_sa(c):
    """(GROUPS, n) per-sample exponents of a PS probe (``sample_prescale``), and the float64 bounds."""
    out = [X.sample_prescale_ref(c["amax"][ga(c, g)], X.bits_f32(c["smax_in"] if c["shared"] else
                                                                  c["smax_in"][g * c["n_win"]:(g + 1) * c["n_win"]]))
           for g in range(GROUPS)]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def probe_model(c, **mut):
    return model(c, sa=probe_sa(c)[0] if c.get("smax_in") is not None else None, **mut)


def probe_exact(c, M):
    """The exactness conditions of a probe's model: every fma exact and staged = hi + lo; every entry's product a
    multiple of its grid unit with the absolute terms below 2^24 units."""
    sa = probe_sa(c)[0] if c.get("smax_in") is not None else None
    for g in range(GROUPS):
        v, aff = group_in(c, g).double(), c["aff"][ga(c, g)].double()
        a64 = torch.where(M["keep"][g], v * aff[0] + aff[1], torch.zeros((), dtype=torch.float64))
        if sa is not None:
            a64 = a64 * torch.pow(2.0, sa[g].double())[:, None, None]
        a, hi, lo = stage(group_in(c, g), c["aff"][ga(c, g)], M["keep"][g], None if sa is None else sa[g])
        if not (torch.equal(a.double(), a64) and torch.equal(hi + lo, a64)):
            return False
    u = c["unit"]
    q = M["core"] / u
    ab = (M["ab"] - torch.stack([c["bias"][gw(c, g)].double().abs() for g in range(GROUPS)])[:, None, None]) / u
    return bool((q == q.round()).all()) and bool((ab < 2.0 ** 24).all())


def lo_share(c, M):
    """Share of the staged elements with lo != 0."""
    sa = probe_sa(c)[0] if c.get("smax_in") is not None else None
    n = sum(int((stage(group_in(c, g), c["aff"][ga(c, g)], M["keep"][g], None if sa is None else sa[g])[2] != 0).sum())
            for g in range(GROUPS))
    return n / (GROUPS * c["n_win"] * L * c["cin"])


def probe_refs(kind, l, n_win, variant):
    """Case and model of one probe, computed once and shared (read-only).  kind: "probe", "ps", "moment"."""
    key = (kind, l, n_win, variant)
    if key not in _cache:
        c = moment_probe_case(l, n_win, variant) if kind == "moment" else probe_case(l, n_win, variant, kind == "ps")
        _cache[key] = dict(c=c, M=probe_model(c))
    return _cache[key]


def probe_cases():
    """(l, n_win, variant): all mask variants and the shared layout at 5 windows, and one variant at the layer's
    dense tile edge (4 rows left in the last tile)."""
    out = []
    for l in LAYERS:
        out += [(l, PROBE_NWIN, v) for v in VARIANTS]
        out.append((l, 15 if tile_rows(l) == 128 else 47, VARIANTS[l % 3]))
    return out


def bits_differ(got, want):
    """Entries of two fp32 tensors whose bit patterns differ."""
    return int((X.f32_bits(got) != X.f32_bits(want)).sum())
