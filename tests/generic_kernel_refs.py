"""float64 CPU references of the generic training kernels, one kernel each (``csrc/generic_conv.hip`` modes
kTrain / kLinear, ``csrc/generic_train.hip``, ``csrc/generic_wgrad.hip``, ``csrc/gf32_conv.hip``), the
per-entry allowances they are compared under, and the fixtures both test files share
(``test_generic_kernel_refs_cpu.py`` checks this oracle without a GPU, ``test_generic_train_kernels_gpu.py``
holds the kernels to it).

Every reference works on the kernel's ACTUAL inputs -- the bf16 (or fp32) values the kernel reads, upcast to
float64 -- so what is left between kernel and reference is fp32 accumulation, a few ulps of ``rsqrtf`` /
``__expf`` and the rounding of the final store.  The allowances are derived from that, per entry:

* ``U32 = 2^-23`` per fp32 addition: twice the unit roundoff, which also covers an MFMA accumulate that
  does not round to nearest;
* ``UB = 2^-8`` for one bf16 store: the unit roundoff of its 8-bit significand (round to nearest).
"""
import atexit
import functools
import json
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.csrc import build
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng

U32 = 2.0 ** -23
UB = 2.0 ** -8
EPS = float(np.float32(1e-3))          # the kernels take eps / momentum as float
MOMENTUM = float(np.float32(0.99))


# ------------------------------------------------------------------------------------------ launch geometry
# Stated once, in csrc/generic_geo.h.  The tests learn it by running the stand-alone host program
# tests/generic_geo_check.cpp (which also checks the header against brute force, test_generic_geo_cpu.py),
# built once per session into a temporary directory.
BF16, GF32 = 0, 1                  # generic_geo.h Engine
INFER, TRAIN, LINEAR = 0, 1, 2     # ... and Mode


@functools.lru_cache(maxsize=None)
def geo_check_exe(name="generic_geo_check", flags=()):
    """tests/<name>.cpp built with the host compiler against csrc/ (once per session)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    tmp = tempfile.mkdtemp(prefix=name + "_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{build.HERE}", *flags,
                        os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@functools.lru_cache(maxsize=None)
def geo_table(what, *args):
    """One launch's plan (``--table``).  ``"conv", engine, mode, n, L, cin, cout, k, pool, in_rs`` -> kind
    ("staged" = conv_lds_kernel, "vec", "elem"), ct, nct, grid, span, lds_rows, lds_stride, lds_bytes,
    nc, ...; ``"wgrad", R, cin, cout, k, part_floats`` (gf32) -> groups, rpg, grid;
    ``"gt_wgrad", R, cin, cout, k, det, part_floats`` -> ok, im2col, nco, kmax, rgs, ...; ``"const"``."""
    r = subprocess.run([geo_check_exe(), "--table", what, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def f64(t):
    return t.detach().cpu().double()


def d64(t):
    """As :func:`f64`, on the tensor's own device (references computed next to the kernels' outputs)."""
    return t.detach().double()


def f32r(t):
    """float64 tensor rounded once to fp32 (and back): what a kernel reads from an fp32 buffer."""
    return t.float().double()


def stored(t, bf16):
    """Round to the storage type of an activation buffer and upcast again."""
    return t.to(torch.bfloat16).double() if bf16 else t.float().double()


# ------------------------------------------------------------------------------------------ convolution
def conv64(x, w, b=None, relu=False, to=f64):
    """(N, L, Cin) x (k, Cin, Cout) 'same' conv in float64 (odd k).  ``to``: :func:`f64` (CPU) or :func:`d64`."""
    xt = to(x).permute(0, 2, 1)
    wt = to(w).permute(2, 1, 0)
    y = torch.nn.functional.conv1d(xt, wt, None if b is None else to(b), padding=(w.shape[0] - 1) // 2)
    y = y.permute(0, 2, 1)
    return torch.relu(y) if relu else y


def conv_abs64(x, w, b=None, to=f64):
    """The abs-sum companion: sum of the absolute terms of every output entry."""
    return conv64(to(x).abs(), to(w).abs(), None if b is None else to(b).abs(), to=to)


def flip_t(w):
    """The dgrad kernel W'[tap][co][ci] = W[k - 1 - tap][ci][co]."""
    return w.flip(0).permute(0, 2, 1).contiguous()


def row_index(n, L, rs, off):
    """Buffer rows of the data rows (s, t), s < n, t < L, in the padded layout s * rs + off + t."""
    return (torch.arange(n)[:, None] * rs + off + torch.arange(L)[None, :]).reshape(-1)


def place_rows(buf, v, rs, off):
    """Write (n, L, C) into ``buf`` (rows, C) at rows s * rs + off + t; returns ``buf``."""
    n, L, _ = v.shape
    buf[row_index(n, L, rs, off)] = v.reshape(n * L, -1).to(buf.dtype)
    return buf


def conv_allow(ref, abs_sum, K, bf16):
    """|y - ref| per entry: one bf16 store + (K + 2) fp32 additions (K products, bias, slack) over the
    absolute terms."""
    a = (K + 2) * U32 * abs_sum
    return a + UB * ref.abs() if bf16 else a


def moments64(u):
    """(2, C): sum u, sum u^2 over the rows of (N, L, C) or (rows, C)."""
    u = u.reshape(-1, u.shape[-1])
    return torch.stack([u.sum(0), (u * u).sum(0)])


def moments_allow(u, e, chain):
    """Allowance of the slot-table sums (2, C) against ``moments64(u)``: ``chain`` fp32 additions on the
    longest chain over the absolute terms (one more for the square's own rounding), plus the conv error
    ``e`` (per entry, no store rounding: the moments come from the unrounded fp32 activation) carried into
    sum u and sum u^2."""
    u, e = u.reshape(-1, u.shape[-1]), e.reshape(-1, e.shape[-1])
    a1 = chain * U32 * u.abs().sum(0) + e.sum(0)
    a2 = (chain + 1) * U32 * (u * u).sum(0) + (2 * u.abs() * e + e * e).sum(0)
    return torch.stack([a1, a2])


def conv_chain(rows, det):
    """fp32 additions on the longest chain of a conv moment: 4 row tiles, 4 steps of the 16-lane tree and,
    in atomic mode, 2 * ceil(grid.x / 16) atomic adds into one slot."""
    gx = -(-rows // 128)
    return 8 + (0 if det else 2 * -(-gx // 16))


# ------------------------------------------------------------------------------------------ BN finalize
def bn_moments64(slots, inv_count):
    """mean, var (clamped at 0) and E[u^2] of an (nslots, 2, C) fp32 slot table, summed in extended
    precision so that the reference adds no error of its own to the cancellation."""
    s = f64(slots).numpy().astype(np.longdouble).sum(0)
    ic = np.longdouble(inv_count)
    mean, eu2 = s[0] * ic, s[1] * ic
    var = np.maximum(eu2 - mean * mean, np.longdouble(0))
    to = lambda a: torch.from_numpy(a.astype(np.float64))
    return to(mean), to(var), to(eu2)


def bn_finalize64(slots, inv_count, gamma, beta, eps, momentum, mmean, mvar):
    """-> (scale, shift, mean, rstd, mmean', mvar') of ``gt_bn_finalize``."""
    mean, var, _ = bn_moments64(slots, inv_count)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = f64(gamma) * rstd
    shift = f64(beta) - mean * scale
    mm = f64(mmean) * momentum + mean * (1.0 - momentum)
    mv = f64(mvar) * momentum + var * (1.0 - momentum)
    return scale, shift, mean, rstd, mm, mv


def bn_finalize_allow(slots, inv_count, gamma, beta, eps, momentum, mmean, mvar):
    """Allowances in the order of :func:`bn_finalize64`.  mean: one fp32 rounding of an fp64 sum.  var: its
    fp32 rounding and the fp64 cancellation of E[u^2] - mean^2.  rstd, scale: the ulps of rsqrtf.  shift and
    the moving averages: 2^-22 of their terms (two fp32 roundings), the variance's own allowance carried."""
    mean, var, eu2 = bn_moments64(slots, inv_count)
    scale, shift, _, rstd, _, _ = bn_finalize64(slots, inv_count, gamma, beta, eps, momentum, mmean, mvar)
    a_var = 2.0 ** -22 * var + 2.0 ** -50 * eu2
    a_mean = 2.0 ** -23 * mean.abs()
    a_mm = 2.0 ** -22 * ((f64(mmean) * momentum).abs() + (mean * (1 - momentum)).abs())
    a_mv = 2.0 ** -22 * ((f64(mvar) * momentum).abs() + (var * (1 - momentum)).abs()) + (1 - momentum) * a_var
    return (2.0 ** -21 * scale.abs(), 2.0 ** -21 * (f64(beta).abs() + (mean * scale).abs()), a_mean,
            2.0 ** -21 * rstd, a_mm, a_mv)


# ------------------------------------------------------------------------------------------ apply
def keep_mask(skey, window_offset, n, lout, C, rate):
    return rng.keep_mask_torch(skey, window_offset + torch.arange(n), lout, C, rate)


def pool_pairs(y):
    lo = y.shape[1] // 2
    return y[:, 0: 2 * lo: 2], y[:, 1: 2 * lo: 2]


def apply64(z, sc, sh, pool, keep=None, inv_keep=1.0):
    """BN affine + valid 2:1 max pool (odd L drops the last step) + inverted dropout of ``gt_apply``.
    -> (y (n, lout, C), mag = inv_keep (|z sc| + |sh|), the magnitude its fp32 roundings act on)."""
    y = z * sc + sh
    mag = (z * sc).abs() + sh.abs()
    if pool:
        ya, yb = pool_pairs(y)
        ma, mb = pool_pairs(mag)
        y, mag = torch.maximum(ya, yb), torch.maximum(ma, mb)
    if keep is not None:
        y = torch.where(keep, y * inv_keep, torch.zeros((), dtype=y.dtype))
        mag = mag * inv_keep
    return y, mag


def apply_allow(ref, mag, bf16):
    a = 2.0 ** -22 * mag
    return a + UB * ref.abs() if bf16 else a


# ------------------------------------------------------------------------------------------ backward
def pool_winner(z, sc, sh, bf16):
    """-> (win, excl), both (n, L // 2, C).  ``win``: the even row of the pair takes the gradient (first
    maximum: ya >= yb).  bf16 storage: decided on the single-rounded fp32 value float32(float64(z) sc + sh),
    bit-equal to the kernel's fmaf whenever the float64 sum is exact (an 8-bit z times a 24-bit scale is).
    ``excl``: pairs with unequal z whose float64 values differ by less than 2^-20 of the larger -- an fp32
    fmaf may order them either way, so they are left out of the comparison; exact ties never are."""
    y = z * sc + sh
    ya, yb = pool_pairs(y)
    za, zb = pool_pairs(z)
    excl = (za != zb) & ((ya - yb).abs() < 2.0 ** -20 * torch.maximum(ya.abs(), yb.abs()))
    if bf16:
        ya, yb = pool_pairs(f32r(y))
    return ya >= yb, excl


def head_upstream64(dlog, w, invL, lout):
    """Head mode: dh[n, t, c] = dlog[n] w[c] invL."""
    return (f64(dlog) * invL)[:, None, None] * f64(w)[None, None, :] * torch.ones(1, lout, 1, dtype=torch.float64)


def upstream64(g, L, pool, keep=None, inv_keep=1.0, win=None):
    """Upstream gradient (n, lout, C) back through the dropout mask and the pool -> dy (n, L, C)."""
    if keep is not None:
        g = torch.where(keep, g * inv_keep, torch.zeros((), dtype=g.dtype))
    if not pool:
        return g
    n, lo, C = g.shape
    full = torch.zeros(n, L, C, dtype=g.dtype)
    zero = torch.zeros((), dtype=g.dtype)
    full[:, 0: 2 * lo: 2] = torch.where(win, g, zero)
    full[:, 1: 2 * lo: 2] = torch.where(win, zero, g)
    return full


def bwd_stats64(z, mean, rstd, dy):
    """-> (sums (2, C): sum dy, sum dy xhat; the sums of their absolute terms)."""
    t = dy * ((z - mean) * rstd)
    return torch.stack([dy.sum((0, 1)), t.sum((0, 1))]), torch.stack([dy.abs().sum((0, 1)), t.abs().sum((0, 1))])


def bwd_finalize64(sums, inv_count):
    """-> (ggamma, gbeta, coef (2, C)) of ``gt_bwd_finalize``."""
    return sums[1], sums[0], sums * inv_count


def bwd_dz64(z, mean, rstd, gamma, dy, k0, k1):
    """dz = relu'(z) gamma rstd (dy - k0 - xhat k1) -> (dz (n, L, C), mag = |gr| (|dy| + |k0| + |xh k1|))."""
    xh = (z - mean) * rstd
    gr = f64(gamma) * rstd
    pos = z > 0
    zero = torch.zeros((), dtype=torch.float64)
    dz = torch.where(pos, gr * (dy - k0 - xh * k1), zero)
    mag = torch.where(pos, gr.abs() * (dy.abs() + k0.abs() + (xh * k1).abs()), zero)
    return dz, mag


def elem_grid(items, per_block):
    return max(1, min(4096, -(-items // per_block)))


def bwd_chain(rows, C, slots, det):
    """fp32 additions on the longest chain of a backward sum (csrc/generic_train.hip bwd_kernel): the rows
    of one thread, the block reduce over the 256 / (C / 4) row lanes, the atomic adds into one of 16 slots
    (deterministic: none, one slot per block, the grid capped at the slot count), + 4 for the roundings
    inside one term (dlog invL, w, inv_keep, (z - mu) rstd, the product: each half of U32)."""
    rpb = 256 // (C // 4)
    g = elem_grid(rows, rpb * 4)
    if det:
        g = min(g, slots)
    return -(-rows // (g * rpb)) + rpb + (0 if det else -(-g // 16)) + 4


def dz_allow(ref, mag, bf16):
    a = 2.0 ** -20 * mag
    return a + UB * ref.abs() if bf16 else a


# ------------------------------------------------------------------------------------------ wgrad / head
def wgrad64(xp, dzp, R, k, to=f64):
    """gw[tap] = xp[tap : tap + R].T @ dzp[:R] -> (gw (k, cin, cout), the same over absolute values)."""
    xp, dzp = to(xp), to(dzp)[:R]
    gw = torch.stack([xp[t: t + R].t() @ dzp for t in range(k)])
    ab = torch.stack([xp[t: t + R].abs().t() @ dzp.abs() for t in range(k)])
    return gw, ab


def head64(h, w, b, y, inv_gb, dlog=None):
    """GAP + Dense + BCE on logits of ``gt_head``; h (n, L, C).  Returns a dict: prob, dlog, loss (summed),
    gw, gb, logit, and the absolute-term sums the allowances need.  prob - y is formed without cancellation
    (a float64 sigmoid(30) - 1 has lost three digits): (1 - y) - sigmoid(-z) for z >= 0.
    ``dlog``: the kernel's own per-sample dlogit (its actual input to the dense gradients); the gradients
    are then sum dlog g and sum dlog of THAT, so that only their own fp32 accumulation is left -- dlog
    itself is held to its allowance separately."""
    h, w, b, y = f64(h), f64(w), f64(b), f64(y)
    g = h.mean(1)
    # the average over time is itself an fp32 sum inside the kernel (not an input): the absolute terms of
    # everything built on it are those of h, mean_t |h|, not |mean_t h|
    ga = h.abs().mean(1)
    z = g @ w + b
    p = torch.sigmoid(z)
    d = torch.where(z >= 0, (1.0 - y) - torch.sigmoid(-z), p - y) * inv_gb
    dg = d if dlog is None else f64(dlog)
    t1, t2, t3 = torch.clamp(z, min=0), z * y, torch.log1p(torch.exp(-z.abs()))
    lv = t1 - t2 + t3
    return dict(prob=p, dlog=d, loss=lv.sum(), gw=(dg[:, None] * g).sum(0), gb=dg.sum(), logit=z,
                logit_abs=ga @ w.abs() + b.abs(), loss_abs=(t1 + t2.abs() + t3).sum(),
                gw_abs=(dg.abs()[:, None] * ga).sum(0), gb_abs=dg.abs().sum())


def head_allow(r, n, C, inv_gb):
    """prob, dlog: 2^-21 relative (the ulps of expf and the divisions) plus the logit's fp32 error,
    2^-22 of the sum of its absolute terms sum |g w| + |b| (the dense bias is one of the terms: the fp32
    logit of a sample planted at 30 cannot be closer than 2^-24 * 30), carried through the sigmoid's largest slope on that interval (dlog = (prob - y) inv_gb:
    times inv_gb).  Relative to dlog itself: a saturated prob must not cancel against its label.
    loss and gradients: (n + C / 64 + 8) fp32 additions over the absolute terms."""
    dz = 2.0 ** -22 * r["logit_abs"]
    za = (r["logit"].abs() - dz).clamp(min=0)
    slope = torch.sigmoid(za) * torch.sigmoid(-za)
    a_prob = 2.0 ** -21 * r["prob"] + slope * dz
    a_dlog = 2.0 ** -21 * r["dlog"].abs() + inv_gb * slope * dz
    cnt = (n + C / 64 + 8) * U32
    return dict(prob=a_prob, dlog=a_dlog, loss=cnt * r["loss_abs"], gw=cnt * r["gw_abs"], gb=cnt * r["gb_abs"])


# ================================================================================================ fixtures
def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (1 << 31))


# (cin, L, k, cout, n): gt_conv mode 1 / mode 2 (+ gt_pack); the path named is the forward launch's
CONV_CASES = [
    (64, 60, 5, 128, 9),    # LDS-staged; cout 128 = one full channel block
    (8, 45, 9, 36, 9),      # LDS-staged; cout 36: last channel tile a quarter full
    (224, 60, 7, 96, 9),    # LDS-staged, 70.5 KB of LDS (just under the 80 KB limit)
    (64, 45, 11, 20, 9),    # LDS-staged, k = 11
    (8, 1, 3, 12, 1),       # LDS-staged, n = 1, L = 1: one row
    (96, 3, 9, 20, 9),      # 16-byte (vector) gather: LDS span 97.5 KB
    (256, 1, 7, 12, 9),     # 16-byte (vector) gather: L = 1, LDS span 462 KB
    (4, 60, 7, 132, 9),     # element gather; cout 132: second channel block (grid.y = 2), 4 channels in it
    (1, 30, 7, 256, 9),     # element gather; cout 256: second channel block, full
    (36, 15, 3, 100, 9),    # element gather; cout 100: not a multiple of 16
    (100, 45, 1, 12, 9),    # element gather, k = 1
]


def conv_fixture(cin, L, k, cout, n):
    """bf16-exact inputs of one conv case, unit-scale output."""
    g = _gen(1, cin, L, k, cout, n)
    x = torch.randn(n, L, cin, generator=g).bfloat16().float()
    w = (torch.randn(k, cin, cout, generator=g) / math.sqrt(k * cin)).float()
    b = (torch.randn(cout, generator=g) * 0.5).float()
    dz = torch.randn(n, L, cout, generator=g).bfloat16().float()
    return x, w, b, dz


# (cin, L, k, cout): gf_conv / gf_wgrad, n = 9
GF_CASES = [
    (1, 30, 7, 96),     # three channel tiles per wave (CT = 3), one input channel
    (3, 45, 15, 100),   # CT = 4, cout not a multiple of 16, k = 15
    (36, 15, 1, 256),   # CT = 4, two channel blocks (grid.y = 2), k = 1, two 32-channel chunks (one partial)
    (64, 60, 7, 96),    # CT = 3, 540 rows: five row blocks
]

# (cin, k, cout, n, L): gt_wgrad; R = n (L + k - 1)
WGRAD_CASES = [
    (1, 7, 12, 9, 30),      # im2col (cin k = 7); nco 1; R = 324, one row group
    (3, 9, 20, 9, 45),      # im2col (cin k = 27); nco 1; R = 477
    (4, 7, 100, 9, 60),     # im2col (cin k = 28); nco 2; R = 594
    (36, 3, 100, 9, 60),    # KMAX 3, element loads; nco 2; R = 558 = 9 chunks: 3 row groups (many)
    (36, 1, 12, 1, 1),      # KMAX 3, k = 1; nco 1; R = 1
    (36, 3, 12, 3, 7),      # KMAX 3; nco 1; R = 27 < 64
    (96, 5, 256, 9, 60),    # KMAX 5, 16-byte loads; nco 4; R = 576 = 9 chunks (a multiple of 64: the even case)
    (224, 9, 192, 9, 15),   # KMAX 9, 16-byte loads; nco 3; R = 207
    (100, 9, 256, 9, 15),   # KMAX 9, element loads (cin 100); nco 2; R = 207
    (36, 11, 20, 9, 45),    # KMAX 15 (k = 11); nco 1; R = 495
    (96, 15, 256, 9, 30),   # KMAX 15 (k = 15); nco 2; R = 396
]


def wgrad_fixture(cin, k, cout, n, L):
    """Every row random (the padding rows too: the reference is the plain row-shifted product)."""
    g = _gen(2, cin, k, cout, n, L)
    R = n * (L + k - 1)
    xp = torch.randn(R + k - 1, cin, generator=g).bfloat16().float()
    dzp = torch.randn(R, cout, generator=g).bfloat16().float()
    return xp, dzp, R


def wgrad_allow(ab, R, extra=16):
    return (R + extra) * U32 * ab


# ---- gt_bn_finalize: slot tables of real fp32 samples
BN_NSLOTS = [16, 17, 255, 256, 257, 258, 319, 320, 321, 385]   # packed two-launch sum from 256; one-slot
BN_C = [4, 20, 100, 1024]                                       # tail (nslots % 64 == 1): 257, 321, 385
BN_COUNTS = [3840, 1665, 4096]
_bn_samples = {}


def bn_samples(C):
    """(4096, C) fp32 samples, as float64: channel 0 all zero (dead ReLU), 1 all equal (the clamp at 0),
    2 mean 100 / std 0.01, 3 mean 5 / std 1e-3, the rest relu(N(0.3, 1)) at mixed scales."""
    if C not in _bn_samples:
        g = _gen(3, C)
        u = torch.relu(torch.randn(4096, C, generator=g) + 0.3) * (0.25 + 4 * torch.rand(C, generator=g))
        u[:, 0] = 0.0
        u[:, 1] = 0.75
        u[:, 2] = 100.0 + 0.01 * torch.randn(4096, generator=g)
        u[:, 3] = 5.0 + 1e-3 * torch.randn(4096, generator=g)
        _bn_samples[C] = u.float().double()
    return _bn_samples[C]


def bn_fixture(nslots, C, count):
    """-> (slots (nslots, 2, C) fp32, gamma, beta, mmean, mvar fp32): the first ``count`` samples split
    into ``nslots`` contiguous runs, each run's two sums rounded to fp32 as a producing kernel stores them."""
    u = bn_samples(C)[:count].numpy()
    starts = (np.arange(nslots) * count) // nslots
    s1 = np.add.reduceat(u, starts, axis=0)
    s2 = np.add.reduceat(u * u, starts, axis=0)
    slots = torch.from_numpy(np.stack([s1, s2], axis=1)).float()
    g = _gen(4, C)
    gamma = (0.5 + torch.rand(C, generator=g)).float()
    beta = (2 * torch.rand(C, generator=g) - 1).float()
    mmean = torch.randn(C, generator=g).float()
    mvar = (0.5 + torch.rand(C, generator=g)).float()
    return slots, gamma, beta, mmean, mvar


# ---- gt_apply / gt_bwd / gt_bwd_finalize
ELEM_C = [4, 12, 36, 100, 256, 1024]            # C = 4: G = 1, rpb = 256; C = 1024: G = 256, rpb = 1
ELEM_NL = [(1, 1), (3, 7), (9, 45), (5, 60)]
# (pool, rate, window_offset): every case runs four of these, rotated by its index, so that every value
# meets every other across the grid
ELEM_VARIANTS = [(False, 0.0, 0), (True, 0.2, 1000), (True, 0.0, 0), (False, 0.5, 0), (True, 0.5, 0),
                 (False, 0.2, 1000), (True, 0.2, 0), (False, 0.5, 1000), (True, 0.5, 1000), (False, 0.2, 0)]
SKEY = rng.stream_key(2025, 3, (1 << 30) + 7)


# G = 1 (C = 4) with enough rows (18000 > 16 * 1024) that a 16-slot deterministic table caps the grid
ELEM_EXTRA = [(True, 4, 300, 60), (False, 4, 300, 60)]


def elem_variants(bf16, C, n, L):
    if (n, L) not in ELEM_NL:
        return [(True, 0.2, 1000), (False, 0.5, 0)]
    i = (ELEM_C.index(C) * len(ELEM_NL) + ELEM_NL.index((n, L))) * 2 + (0 if bf16 else 1)
    return [ELEM_VARIANTS[(3 * i + j) % len(ELEM_VARIANTS)] for j in range(4)]


def inv_keep(rate):
    return float(np.float32(1.0 / (1.0 - rate))) if rate < 1.0 else 0.0


def elem_fixture(bf16, C, n, L, pool, rate, woff, head=False):
    """Inputs (float64 views of what the kernels read) and references of one elementwise case.
    z: unit scale, post-ReLU (half zeros: exact ties in the pool), equal non-zero pairs planted;
    gamma in [0.5, 1.5], |beta| <= 1; bn = (scale, shift, mean, rstd) fp32 of z's own moments."""
    g = _gen(5, bf16, C, n, L, pool, int(rate * 10), woff, head)
    r = torch.randn(n, L, C, generator=g)
    # positive values start at 0.05: two different bf16 values then differ by >= 2^-8 * 0.05, far more than
    # 2^-20 of any BN output here, so that no bf16 pair is excluded
    z = stored(torch.where(r > 0, 0.05 + 1.5 * r, torch.zeros(())), bf16)
    if L >= 2:
        z[:, 1, : max(1, C // 2)] = z[:, 0, : max(1, C // 2)]   # planted ties, most of them non-zero
    gamma = (0.5 + torch.rand(C, generator=g)).float().double()
    beta = (2 * torch.rand(C, generator=g) - 1).float().double()
    mean = f32r(z.mean((0, 1)))
    var = z.var((0, 1), unbiased=False)
    rstd = f32r(1.0 / torch.sqrt(var + EPS))
    sc = f32r(gamma * rstd)
    sh = f32r(beta - mean * sc)
    lout = L // 2 if pool else L
    ik = inv_keep(rate)
    keep = keep_mask(SKEY, woff, n, lout, C, rate) if rate > 0 else None
    F = dict(z=z, gamma=gamma, beta=beta, bn=torch.stack([sc, sh, mean, rstd]), lout=lout, ik=ik, keep=keep,
             thr=rng.dropout_threshold(rate), n=n, L=L, C=C, pool=pool, rate=rate, woff=woff, bf16=bf16)
    F["y"], F["ymag"] = apply64(z, sc, sh, pool, keep, ik)
    # upstream gradient: a tensor of the storage type, or the head's dlog[n] w[c] invL
    if head:
        F["dlog"] = (torch.randn(n, generator=g) * 0.1).float().double()
        F["w"] = torch.randn(C, generator=g).float().double()
        F["invL"] = float(np.float32(1.0 / max(lout, 1)))
        up = head_upstream64(F["dlog"], F["w"], F["invL"], lout).expand(n, lout, C)
    else:
        F["dh"] = up = stored(torch.randn(n, lout, C, generator=g), bf16)
    if pool:
        F["win"], F["excl"] = pool_winner(z, sc, sh, bf16)
    else:
        F["win"], F["excl"] = None, torch.zeros(n, 0, C, dtype=torch.bool)
    dy = upstream64(up, L, pool, keep, ik, F["win"])
    F["dy"] = dy
    F["sums"], F["sums_abs"] = bwd_stats64(z, mean, rstd, dy)
    F["inv_count"] = 1.0 / (n * L)
    gg, gb, coef = bwd_finalize64(F["sums"], F["inv_count"])
    F["ggamma"], F["gbeta"] = gg, gb
    F["coef"] = f32r(coef)   # what the dz launch reads: its own fp32 inputs
    F["dz"], F["dzmag"] = bwd_dz64(z, mean, rstd, gamma, dy, F["coef"][0], F["coef"][1])
    return F


def excluded_rows(F):
    """(n, L, C) bool: the pre-pool rows of the excluded pool pairs."""
    ex = torch.zeros(F["n"], F["L"], F["C"], dtype=torch.bool)
    if F["pool"]:
        lo = F["lout"]
        ex[:, 0: 2 * lo: 2] = F["excl"]
        ex[:, 1: 2 * lo: 2] = F["excl"]
    return ex


# ---- gt_head: (C, L, n); every value of C in {1, 12, 96, 256, 4096}, L in {1, 3, 60}, n in {1, 3, 4, 5, 130}
HEAD_BIASES = [0.25, 30.0, -30.0]
HEAD_CASES = [(1, 1, 1), (1, 60, 130), (12, 3, 3), (12, 60, 5), (96, 60, 4), (96, 1, 130), (96, 3, 1),
              (256, 3, 130), (256, 60, 5), (4096, 1, 5), (4096, 3, 4), (4096, 60, 3)]


def head_fixture(C, L, n, bf16):
    """h of the storage type, unit-scale GAP . Dense sums, labels 0 / 1.  The tests run each case with the
    dense biases ``HEAD_BIASES``: the large ones plant every logit at about +-30, where the sigmoid
    saturates and the loss is log1pf(exp(-|z|))."""
    g = _gen(6, C, L, n, bf16)
    h = stored(torch.randn(n, L, C, generator=g), bf16)
    w = (torch.randn(C, generator=g) / math.sqrt(C)).float().double()
    y = (torch.rand(n, generator=g) > 0.5).double()
    return h, w, y
