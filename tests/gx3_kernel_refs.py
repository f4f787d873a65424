"""References of the fp16x3 layer-wise kernels (``csrc/gx3_conv.hip``: ``wmax_kernel`` + ``pack_kernel``,
``amax_kernel``, ``conv_kernel<MODE, CT, HALO, VEC>``, ``wgrad_kernel<K>``), one kernel each, in three tiers,
with the per-entry allowances between the tiers and the fixtures both test files share
(``test_gx3_kernel_refs_cpu.py`` checks this oracle without a GPU, ``test_gx3_kernels_gpu.py`` holds the
kernels to it).

1. :func:`split` / :func:`prescale_exp`: the fp16 halves of ``csrc/f16x3.h`` in torch on the CPU.
2. The ARITHMETIC MODEL (:func:`conv_model`, :func:`wgrad_model`): in float64 the sum of hi hi + lo hi + hi lo
   of the halves at the launcher's own prescales (per tensor ``sw``; per 128-row workgroup ``sb`` from the
   samples its rows belong to; the wgrad's ``sx`` / ``sd`` from the amax words handed in), unscaled.  What is
   left between a kernel and its model is fp32 accumulation alone.
3. Plain float64 TRUTH (``generic_kernel_refs.conv64`` / ``wgrad64``) of the fp32 operands.

Allowances (derived, per entry; ``U32 = 2^-23`` per fp32 addition as in ``generic_kernel_refs``):

* kernel against model, :func:`acc_allow`: three MFMAs per k-step, each of the K products counted as one
  addition, + bias + slack -> ``(3 K + 2) U32`` over the absolute terms of the model.
* model against truth, :func:`truth_allow`.  With a = v 2^s = hi + lo + r, fp16 (11-bit significand, normal
  from 2^-14, subnormal spacing 2^-24) gives |lo| <= 2^-11 |a| and |r| <= 2^-11 |lo| <= 2^-22 |a| while lo
  is normal, |r| <= 2^-25 (half the subnormal spacing) once lo -- or hi itself -- is subnormal:
  ``|r| <= max(2^-22 |a|, 2^-25)`` (:data:`SPLIT_REL`, :data:`SPLIT_FLOOR`; asserted on the CPU).  A product
  x w is replaced by X W - xl wl (X = xh + xl): the error is X rw + rx W + rx rw + xl wl, i.e. three terms of
  2^-22 |x w| (two residuals and the dropped lo lo) plus the floors 2^-25 2^-sb |w| and 2^-25 2^-sw |x|, plus
  2^-50 2^-(sb + sw) where both floors meet; the second-order products of these are below 2^-10 of them
  and are covered by the factor 1.01.  Since max 2^s >= 2^13, the floor of one product is at most
  2^-38 max|x| |w|: ABSOLUTE in the workgroup's (conv) or tensor's (wgrad) maximum.  An element below
  2^-16 of that maximum has a subnormal lo and loses relative precision to this floor (2^-8 relative at
  2^-30 of the maximum).
"""
import math

import torch

from . import generic_kernel_refs as G
from .generic_kernel_refs import U32, conv64, conv_abs64, f64, flip_t, wgrad64  # noqa: F401  (re-exported)

SPLIT_REL = 2.0 ** -22     # |a - hi - lo| <= SPLIT_REL |a| while lo is a normal fp16
SPLIT_FLOOR = 2.0 ** -25   # ... and <= this (half the fp16 subnormal spacing) otherwise
SLACK = 1.01               # second-order terms of truth_allow


# ================================================================================================ tier 1
def prescale_exp(bound):
    """``csrc/f16x3.h:prescale_exp``: the s that puts ``bound`` into [2^13, 2^14); 0, inf, NaN -> 14."""
    bound = float(bound)
    e = 0
    if bound > 0.0 and math.isfinite(bound):
        e = math.frexp(bound)[1]
    return min(100, max(-100, 14 - e))


def split(v, s):
    """fp32 v -> (hi, lo) fp16: hi = fp16(v 2^s), lo = fp16(fp32(v 2^s) - hi), round to nearest even,
    subnormals honoured (torch on the CPU)."""
    a = (v.detach().cpu().double() * 2.0 ** s).float()   # one rounding: the fp32 product by a power of two
    hi = a.half()
    lo = (a - hi.float()).half()
    return hi, lo


def halves64(v, s):
    """The halves as float64, unscaled: (hi 2^-s, lo 2^-s)."""
    hi, lo = split(v, s)
    return hi.double() * 2.0 ** -s, lo.double() * 2.0 ** -s


def amax32(t):
    """max |t| as the fp32 value a kernel publishes (0 for an empty / all-zero tensor)."""
    return float(t.detach().float().abs().max()) if t.numel() else 0.0


def bits(v):
    """int32 bit pattern of one fp32 value (the amax words)."""
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item())


# ================================================================================================ launcher mirror
def conv_path(n, L, cin, cout, k, in_rs=None):
    """What ``launch_gx3_conv`` selects for one launch (a restatement, checked by the CPU tests against the
    figures each case is named for)."""
    p = (k - 1) // 2
    in_rs = L + 2 * p if in_rs is None else in_rs
    rows = n * L
    nct = (cout + 15) // 16
    tap0, tap1 = max(p - (L - 1), 0), min(p + L, k)
    span = 128 + (127 + L - 1) // L * max(in_rs - L, 0) + 2 * p
    halo = cin % 32 == 0 and span * 8 <= 256 * 8
    ct = 3 if nct % 6 == 0 else 4
    gy = -(-nct // (2 * ct))
    # channel tiles of each (workgroup column, wave column): min(CT, nct - ct0) where active
    nc = [[max(0, min(ct, nct - (by * 2 + wc) * ct)) for wc in range(2)] for by in range(gy)]
    return dict(path="halo" if halo else "vec" if cin % 8 == 0 else "elem", halo=halo, CT=ct, nct=nct,
                grid=(-(-rows // 128), gy), span=span if halo else 0, lds=2 * (span if halo else 128) * 160,
                tap0=tap0, tap1=tap1, s0=tap0 * cin // 32, s1=(tap1 * cin + 31) // 32,
                nstep=(k * cin + 31) // 32, nc=nc, last_tile=cout - 16 * (nct - 1), rows=rows)


def wgrad_path(R, cin, cout, k, part_floats):
    """Row groups ``launch_gx3_wgrad`` picks: (groups, rows per group); groups = 0: rejected."""
    wfl = k * cin * cout
    groups = part_floats // wfl
    ci_t, co_g = (cin + 31) // 32, (cout + 63) // 64
    want = min((512 + ci_t * co_g - 1) // (ci_t * co_g), (R + 255) // 256)
    groups = min(groups, want, 65535)
    if groups < 1:
        return 0, 0
    rpg = -(-(-(-R // groups)) // 64) * 64
    return -(-R // rpg), rpg


def tiles(x, L):
    """The 128-row workgroups of a conv over x (n, L, cin): [(r0, r1, n0, n1, sb)], sb from max |x| over the
    samples n0 .. n1 the rows belong to."""
    n = x.shape[0]
    rows = n * L
    out = []
    for r0 in range(0, rows, 128):
        r1 = min(r0 + 128, rows)
        n0, n1 = r0 // L, (r1 - 1) // L
        out.append((r0, r1, n0, n1, prescale_exp(amax32(x[n0: n1 + 1]))))
    return out


# ================================================================================================ tier 2
def conv_model(x, w, b=None, relu=False, drop=(), exps=None):
    """The conv kernel's arithmetic in float64.  x (n, L, cin), w (k, cin, cout) fp32 (dgrad: dz and
    ``flip_t(w)``).  -> dict: ``y`` (rows, cout); ``ab`` the sum of the absolute terms (bias included);
    ``sb`` (rows,) the prescale of each row's workgroup; ``sw``.
    ``drop``: names of terms left out ("lo_hi" = w.lo x.hi, "hi_lo" = w.hi x.lo) and ``exps``: a replacement
    for the per-tile exponents -- the mutations of the CPU self-check."""
    n, L, _ = x.shape
    cout = w.shape[2]
    rows = n * L
    sw = prescale_exp(amax32(w))
    wh, wl = halves64(w, sw)
    T = tiles(x, L)
    sbs = [t[4] for t in T] if exps is None else list(exps)
    y = torch.zeros(rows, cout, dtype=torch.float64)
    ab = torch.zeros(rows, cout, dtype=torch.float64)
    sb_row = torch.zeros(rows, dtype=torch.float64)
    for sb in sorted(set(sbs)):
        xh, xl = halves64(x, sb)
        terms = [(xh, wh)]
        if "lo_hi" not in drop:
            terms.append((xh, wl))
        if "hi_lo" not in drop:
            terms.append((xl, wh))
        yy = sum(conv64(a, c) for a, c in terms).reshape(rows, cout)
        aa = sum(conv_abs64(a, c) for a, c in terms).reshape(rows, cout)
        for (r0, r1, _, _, _), s in zip(T, sbs):
            if s == sb:
                y[r0:r1], ab[r0:r1], sb_row[r0:r1] = yy[r0:r1], aa[r0:r1], sb
    if b is not None:
        y = y + f64(b)
        ab = ab + f64(b).abs()
    if relu:
        y = torch.relu(y)
    return dict(y=y, ab=ab, sb=sb_row, sw=sw)


def acc_allow(ab, K, extra=2):
    """Kernel against model: (3 K + extra) fp32 additions over the absolute terms."""
    return (3 * K + extra) * U32 * ab


def conv_truth(x, w, b=None, relu=False):
    return conv64(x, w, b, relu).reshape(-1, w.shape[2])


def truth_allow(x, w, sb_row, sw):
    """Model against truth, per entry (rows, cout); see the module docstring."""
    cout = w.shape[2]
    rows = x.shape[0] * x.shape[1]
    one_x, one_w = torch.ones_like(f64(x)), torch.ones_like(f64(w))
    prod = conv_abs64(x, w).reshape(rows, cout)
    sum_w = conv64(one_x, f64(w).abs()).reshape(rows, cout)       # over the taps inside the sample
    sum_x = conv64(f64(x).abs(), one_w).reshape(rows, cout)
    cnt = conv64(one_x, one_w).reshape(rows, cout)
    fb = (2.0 ** -sb_row)[:, None]
    fw = 2.0 ** -sw
    return SLACK * (3 * SPLIT_REL * prod + SPLIT_FLOOR * (fb * sum_w + fw * sum_x) + SPLIT_FLOOR ** 2 * fb * fw * cnt)


def wgrad_model(xp, dzp, R, k, ax, ad, drop=(), rows=None):
    """The wgrad kernel's arithmetic in float64: gw[tap] = sum_r x[r + tap] dz[r] over the halves at
    sx = prescale_exp(ax), sd = prescale_exp(ad) (the amax words handed in, as fp32 values).
    ``rows``: the dz rows summed (default all R) -- the dropped row group of the CPU self-check."""
    sx, sd = prescale_exp(ax), prescale_exp(ad)
    xh, xl = halves64(xp, sx)
    dh, dl = halves64(dzp[:R], sd)
    if rows is not None:
        keep = torch.zeros(R, 1, dtype=torch.float64)
        keep[rows] = 1.0
        dh, dl = dh * keep, dl * keep
    terms = [(xh, dh)]
    if "lo_hi" not in drop:
        terms.append((xl, dh))
    if "hi_lo" not in drop:
        terms.append((xh, dl))
    gw = torch.stack([sum(a[t: t + R].t() @ c for a, c in terms) for t in range(k)])
    ab = torch.stack([sum(a[t: t + R].abs().t() @ c.abs() for a, c in terms) for t in range(k)])
    return dict(gw=gw, ab=ab, sx=sx, sd=sd)


def wgrad_truth_allow(xp, dzp, R, k, sx, sd):
    xa, da = f64(xp).abs(), f64(dzp)[:R].abs()
    prod = torch.stack([xa[t: t + R].t() @ da for t in range(k)])
    sum_d = da.sum(0)[None, None, :]
    sum_x = torch.stack([xa[t: t + R].sum(0) for t in range(k)])[:, :, None]
    fx, fd = 2.0 ** -sx, 2.0 ** -sd
    return SLACK * (3 * SPLIT_REL * prod + SPLIT_FLOOR * (fx * sum_d + fd * sum_x) + SPLIT_FLOOR ** 2 * fx * fd * R)


def slot_moments(u, rows_per_slot=64):
    """(nslots, 2, C): the deterministic slot table, one slot per (workgroup, wave row) = 64 output rows."""
    rows, C = u.shape
    ns = 2 * -(-rows // 128)
    pad = torch.zeros(ns * rows_per_slot, C, dtype=u.dtype)
    pad[:rows] = u
    pad = pad.view(ns, rows_per_slot, C)
    return torch.stack([pad.sum(1), (pad * pad).sum(1)], 1)


# ================================================================================================ pack
def frag_order(w2d):
    """(K, M) -> (nstep, nct, 64, 8) in the A-fragment order of the 16x16x32 MFMA: lane (m = lane % 16,
    h = lane / 16) of tile ct holds k = 32 s + 8 h + j, j < 8, of channel 16 ct + m; zero past K and M."""
    K, M = w2d.shape
    ns, nct = (K + 31) // 32, (M + 15) // 16
    A = torch.zeros(ns * 32, nct * 16, dtype=w2d.dtype)
    A[:K, :M] = w2d
    return A.view(ns, 4, 8, nct, 16).permute(0, 3, 1, 4, 2).reshape(ns, nct, 64, 8).contiguous()


def pack_ref(w, dgrad):
    """-> (fragments (nstep, nct, 2, 64, 8) fp16 as int16 bits, sw) of w (k, cin, cout), or of the flipped,
    transposed kernel."""
    sw = prescale_exp(amax32(w))
    ww = flip_t(w) if dgrad else w
    hi, lo = split(frag_order(ww.reshape(-1, ww.shape[2]).float()), sw)
    return torch.stack([hi, lo], 2).view(torch.int16), sw


def frag_numel(k, cin, cout):
    return 2 * ((k * cin + 31) // 32) * 512 * ((cout + 15) // 16)


PACK_BLOCKS = [(7, 3, 20), (5, 20, 36), (1, 36, 100), (3, 8, 12), (3, 8, 12), (3, 8, 12), (3, 8, 12), (3, 8, 12)]


def pack_weights():
    """One tensor per ``PACK_BLOCKS`` entry: three random ones; all zero; maximum exactly 2^-3; one float
    below 2^-3; maxima near 1e-35 and 3e35 (both clamps of the prescale; at 3e35 the clamp leaves hi
    infinite, which the kernel and :func:`split` agree on)."""
    g = G._gen(11)
    ws = [torch.randn(k, ci, co, generator=g) for k, ci, co in PACK_BLOCKS]
    below = float(torch.nextafter(torch.tensor(0.125), torch.tensor(0.0)))
    ws[3] = torch.zeros_like(ws[3])
    for i, mx in ((4, 0.125), (5, below), (6, 1e-35), (7, 3e35)):
        u = (torch.rand(PACK_BLOCKS[i], generator=g) * 2 - 1)
        u = u / u.abs().max()
        ws[i] = (u.double() * mx).float()
        ws[i][1, 3, 5] = -mx
    return ws


# ================================================================================================ fixtures
N = 9
# (cin, L, k, cout, n): the path named is the forward launch's (conv_path; asserted by the tests)
CONV_CASES = [
    (64, 60, 5, 128, N),    # HALO, CT = 4, both wave columns full
    (32, 60, 7, 96, N),     # HALO, CT = 3
    (32, 15, 9, 36, N),     # HALO, span 208 = 66,560 B (> 64 KB); nc 3 < CT; last tile a quarter full
    (32, 9, 9, 48, N),      # HALO, span 256 (the limit) = 81,920 B
    (224, 60, 7, 132, N),   # HALO, grid.y = 2, 4 channels in the second column (nc = 1 < CT)
    (32, 8, 9, 48, N),      # IM2COL VEC: span 264, one step past the HALO limit
    (96, 3, 9, 20, N),      # IM2COL VEC: L < k, tap0 = 2
    (256, 1, 7, 12, N),     # IM2COL VEC: L = 1, the centre tap only
    (8, 45, 9, 100, N),     # IM2COL VEC
    (4, 60, 7, 256, N),     # element gather; grid.y = 2, both full
    (1, 30, 7, 96, N),      # element gather; CT = 3; no dgrad
    (36, 15, 3, 100, N),    # element gather; s0 .. s1 with k-steps that straddle taps
    (100, 45, 1, 12, N),    # element gather, k = 1
    (8, 1, 3, 12, 1),       # one-row launch
]
# what each case is named for: (path, CT, grid, span, lds bytes) -- worked out from launch_gx3_conv by hand
CONV_EXPECT = {
    (64, 60, 5, 128, N): ("halo", 4, (5, 1), 144, 46080),
    (32, 60, 7, 96, N): ("halo", 3, (5, 1), 152, 48640),
    (32, 15, 9, 36, N): ("halo", 4, (2, 1), 208, 66560),
    (32, 9, 9, 48, N): ("halo", 4, (1, 1), 256, 81920),
    (224, 60, 7, 132, N): ("halo", 4, (5, 2), 152, 48640),
    (32, 8, 9, 48, N): ("vec", 4, (1, 1), 0, 40960),
    (96, 3, 9, 20, N): ("vec", 4, (1, 1), 0, 40960),
    (256, 1, 7, 12, N): ("vec", 4, (1, 1), 0, 40960),
    (8, 45, 9, 100, N): ("vec", 4, (4, 1), 0, 40960),
    (4, 60, 7, 256, N): ("elem", 4, (5, 2), 0, 40960),
    (1, 30, 7, 96, N): ("elem", 3, (3, 1), 0, 40960),
    (36, 15, 3, 100, N): ("elem", 4, (2, 1), 0, 40960),
    (100, 45, 1, 12, N): ("elem", 4, (4, 1), 0, 40960),
    (8, 1, 3, 12, 1): ("vec", 4, (1, 1), 0, 40960),
}


def conv_fixture(cin, L, k, cout, n):
    """Full-precision fp32 inputs (24 significant bits: both halves in play), unit-scale output."""
    g = G._gen(12, cin, L, k, cout, n)
    x = torch.randn(n, L, cin, generator=g)
    w = torch.randn(k, cin, cout, generator=g) / math.sqrt(k * cin)
    b = torch.randn(cout, generator=g) * 0.5
    dz = torch.randn(n, L, cout, generator=g)
    return x, w, b, dz


_cache = {}


def conv_refs(case):
    """Model, truth and allowances of one random case, computed once and shared (read-only)."""
    if case not in _cache:
        cin, L, k, cout, n = case
        x, w, b, dz = conv_fixture(*case)
        M = conv_model(x, w, b, relu=True)
        r = dict(x=x, w=w, b=b, dz=dz, fwd=M, fwd_truth=conv_truth(x, w, b, True),
                 fwd_a1=acc_allow(M["ab"], k * cin), fwd_a2=truth_allow(x, w, M["sb"], M["sw"]))
        if cin % 4 == 0:
            wf = flip_t(w)
            D = conv_model(dz, wf)
            r.update(dgr=D, dgr_truth=conv_truth(dz, wf), dgr_a1=acc_allow(D["ab"], k * cout, extra=1),
                     dgr_a2=truth_allow(dz, wf, D["sb"], D["sw"]))
        _cache[case] = r
    return _cache[case]


# ---- mixed magnitudes: windows of one tile scaled by 2^(0, 12, -18, 5, -7); L = 15: the first workgroup
# holds samples 0 .. 8, the second the tail of sample 8 alone
MIXED_EXPS = (0, 12, -18, 5, -7)
MIXED_CASES = [(32, 15, 9, 36, N), (8, 15, 5, 48, N), (36, 15, 3, 100, N)]   # HALO, VEC, element gather
MIXED_DZ_SHIFT = -20   # dz sits 2^-20 below x: the wgrad's two tensor maxima are far apart


def mixed_scales(n, rot=0):
    return torch.tensor([2.0 ** MIXED_EXPS[(s + rot) % len(MIXED_EXPS)] for s in range(n)])


def mixed_fixture(cin, L, k, cout, n):
    x, w, b, dz = conv_fixture(cin, L, k, cout, n)
    x = x * mixed_scales(n)[:, None, None]
    dz = dz * (mixed_scales(n, 2) * 2.0 ** MIXED_DZ_SHIFT)[:, None, None]
    return x, w, b, dz


def padded(v, k, fwd):
    """(n, L, C) -> the zero-padded row buffer of ops/generic_train.py, in_rs = L + 2 p.  ``fwd``: a forward
    input, 2 p + n in_rs rows, sample s at rows 2 p + s in_rs + t (in_off = 2 p; as the wgrad's Xpad, row
    r + tap meets dZpad's row r); else a dgrad input / dZpad, n in_rs rows, in_off = p."""
    n, L, C = v.shape
    p = (k - 1) // 2
    rs = L + 2 * p
    buf = torch.zeros((2 * p if fwd else 0) + n * rs, C, dtype=v.dtype)
    return G.place_rows(buf, v, rs, 2 * p if fwd else p)


# ---- neighbour independence: 16-bit integers on the 2^-12 grid times per-window factors within 2^+-5
NEIGHBOUR_EXPS = (0, 5, -5, 3, -2, 1, -4, 4, -1)


def neighbour_fixture(cin, L, k, cout, n):
    g = G._gen(13, cin, L, k, cout, n)
    x = torch.randint(-(1 << 15) + 1, 1 << 15, (n, L, cin), generator=g).float() * 2.0 ** -12
    x = x * torch.tensor([2.0 ** NEIGHBOUR_EXPS[s % 9] for s in range(n)])[:, None, None]
    _, w, b, _ = conv_fixture(cin, L, k, cout, n)
    return x, w, b


def split_is_scale_free(v, exps):
    """True when the halves of v are the same fp32 values at every exponent in ``exps`` and lose nothing."""
    e0 = exps[0]
    h0, l0 = halves64(v, e0)
    if not torch.equal(h0 + l0, f64(v)):
        return False
    return all(torch.equal(halves64(v, e)[0], h0) and torch.equal(halves64(v, e)[1], l0) for e in exps[1:])


# ---- exact-arithmetic probes: every half exactly representable at every exponent in play, every product
# and every partial sum a multiple of 2^-PROBE_G below 2^(24 - PROBE_G) in magnitude: exact in fp32 in any order
PROBE_G = 13
PROBE_NNZ = 64             # non-zero weights per dot product: 64 * (15 + 3 2^-13) * (2 + 2^-11) + 8 < 2^11
_PROBE_W = (1.0, -1.0, 2.0, -2.0, 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -12))


def probe_acts(n, L, C, seed):
    """H + l: H an integer 1 .. 15 with a sign (on the fp16 grid), l = j 2^-13 of the same sign, j 1 .. 3: below
    half an fp16 ulp of any H and away from zero (|H + l| stays in H's binade, where H is on the grid), so
    hi = H and lo = l at every prescale that keeps l normal."""
    g = G._gen(14, n, L, C, seed)
    sign = (torch.randint(0, 2, (n, L, C), generator=g) * 2 - 1).double()
    H = torch.randint(1, 16, (n, L, C), generator=g).double()
    j = torch.randint(1, 4, (n, L, C), generator=g).double()
    return (sign * (H + j * 2.0 ** -13)).float()


def probe_nets(k, cin, cout, dgrad):
    """Sparse kernels of +-1, +-2, +-(1 + 2^-12) (hi and lo both non-zero: hi 1, lo 2^-12): at most
    ``PROBE_NNZ`` non-zeros in any forward (and, with ``dgrad``, any dgrad) dot product, and every
    (tap, ci) row -- with ``dgrad`` every (tap, co) row too -- non-zero in at least one net."""
    m = -(-k * (max(cin, cout) if dgrad else cin) // PROBE_NNZ)
    step = min(cin, cout) if dgrad else cout
    tap, ci, co = torch.meshgrid(torch.arange(k), torch.arange(cin), torch.arange(cout), indexing="ij")
    vals = torch.tensor(_PROBE_W)[(tap + 3 * ci + 7 * co) % 6]
    nets = []
    for j in range(-(-m // step)):
        on = (tap * 5 + ci + co + j * step) % m == 0
        nets.append(torch.where(on, vals, torch.zeros(())).float().contiguous())
    return nets


def probe_sparse_dz(R, cout, seed):
    """dz of the wgrad probe: the values of ``_PROBE_W`` on at most 64 rows of every column."""
    m = -(-R // PROBE_NNZ)
    r, co = torch.meshgrid(torch.arange(R), torch.arange(cout), indexing="ij")
    vals = torch.tensor(_PROBE_W)[(r * 5 + co + seed) % 6]
    return torch.where((r + co) % m == 0, vals, torch.zeros(())).float().contiguous()


def is_exact(y, ab):
    """The exactness condition per entry: multiples of 2^-G whose absolute terms sum below 2^(24 - G)."""
    s = y * 2.0 ** PROBE_G
    return bool((s == s.round()).all()) and bool((ab * 2.0 ** PROBE_G < 2.0 ** 24).all())


def probe_bias(cout):
    return ((torch.arange(cout) % 17) - 8).float()


# ---- wgrad: (cin, k, cout, n, L, slices): R = n (L + k - 1); part holds ``slices`` (k, cin, cout) slices
WGRAD_CASES = [
    (1, 7, 12, N, 30, 64),      # K 7; element loads; cout 12: the second wave pair inactive; R = 324
    (3, 15, 48, N, 30, 64),     # K 15; element loads; cout 48; R = 396
    (36, 3, 100, N, 60, 64),    # K 3; second ci tile with 4 channels; second co group, partly active; R = 558: 3 groups
    (36, 3, 100, N, 60, 1),     # the same with part of exactly one slice: one group over 9 chunks
    (36, 1, 12, 1, 1, 1),       # K 1; R = 1
    (36, 5, 12, 3, 7, 64),      # K 5; R = 33 < 64
    (100, 9, 256, N, 15, 64),   # K 9; cin 100; cout 256; R = 207
    (224, 11, 48, N, 45, 64),   # K 11; cin 224; R = 495
    (96, 5, 256, N, 60, 64),    # R = 576 = 3 groups x 192 rows: a multiple of 64 and of the rows per group
]
WGRAD_EXPECT = {   # (groups, rows per group)
    (1, 7, 12, N, 30, 64): (2, 192), (3, 15, 48, N, 30, 64): (2, 256), (36, 3, 100, N, 60, 64): (3, 192),
    (36, 3, 100, N, 60, 1): (1, 576), (36, 1, 12, 1, 1, 1): (1, 64), (36, 5, 12, 3, 7, 64): (1, 64),
    (100, 9, 256, N, 15, 64): (1, 256), (224, 11, 48, N, 45, 64): (2, 256), (96, 5, 256, N, 60, 64): (3, 192),
}


def wgrad_fixture(cin, k, cout, n, L):
    """Every row random, the padding rows too (the reference is the plain row-shifted product), full fp32
    significands."""
    g = G._gen(15, cin, k, cout, n, L)
    R = n * (L + k - 1)
    return torch.randn(R + k - 1, cin, generator=g), torch.randn(R, cout, generator=g), R


def wgrad_acc_allow(ab, R, groups):
    return (3 * R + groups + 2) * U32 * ab


def wgrad_refs(case):
    key = ("w",) + case
    if key not in _cache:
        cin, k, cout, n, L, slices = case
        xp, dzp, R = wgrad_fixture(cin, k, cout, n, L)
        groups, _ = wgrad_path(R, cin, cout, k, slices * k * cin * cout)
        out = dict(xp=xp, dzp=dzp, R=R, groups=groups, truth=wgrad64(xp, dzp, R, k)[0])
        for tag, up in (("", 1.0), ("_up", 2.0 ** 10)):
            ax, ad = amax32(xp) * up, amax32(dzp) * up
            M = wgrad_model(xp, dzp, R, k, ax, ad)
            out.update({"ax" + tag: ax, "ad" + tag: ad, "model" + tag: M,
                        "a1" + tag: wgrad_acc_allow(M["ab"], R, groups),
                        "a2" + tag: wgrad_truth_allow(xp, dzp, R, k, M["sx"], M["sd"])})
        _cache[key] = out
    return _cache[key]


# ---- amax
AMAX_N = [1, 3, 4, 1027]


def ratio(err, allow):
    """Largest |err| / allowance (inf where the allowance is 0 and the error is not, or the error is NaN)."""
    err, allow = err.abs().reshape(-1).double(), allow.reshape(-1).double()
    if not err.numel():
        return 0.0
    inf = torch.full_like(err, float("inf"))
    r = torch.where(allow > 0, err / allow.clamp(min=1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), inf, r)
    return float(r.max())
