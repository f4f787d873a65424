"""float64 references of the dedicated training kernels, one kernel each (``csrc/train_fwd.hip``, ``train_head.hip``,
``train_dgrad.hip``, ``train_wgrad.hip``, ``train_reduce.hip``: forward, parameter table, head, dgrad, wgrad, finalize), the per-entry allowances
they are compared under, and the fixtures both test files share (``test_train_kernel_refs_cpu.py`` checks
this oracle without a GPU, ``test_train_kernels_gpu.py`` holds the kernels to it).

As in ``generic_kernel_refs`` (whose helpers are reused, not copied) every reference works on the kernel's
ACTUAL inputs upcast to float64 -- bf16 activations with the dropout mask in their sign bit, fp32 parameters
and table rows, fp64 moment slots -- so what is left between kernel and reference is fp32 accumulation
(``U32 = 2^-23`` per addition), a few ulps of ``rsqrtf`` / ``expf`` and one bf16 store (``UB = 2^-8``).

These kernels also round INSIDE: the staging of a conv input applies ``A = bf16(fma(|r|, s, t))``
(``decode_pair``).  That rounding is reproduced from the kernel's own fp32 ``s``, ``t`` (:func:`stage64`),
not absorbed into the allowance; only where the float64 value lies within fp32 rounding of a bf16 rounding
boundary is the allowance of exactly the output entries reading that element widened by its bf16 ulp times
``|w|``.  Everything is computed in torch float64 on the device of its inputs; ``rnd=False`` switches every
internal rounding off (the composed step then equals float64 autograd, see the CPU tests).
"""
import functools
import json
import math
import subprocess

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.csrc import build
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import DEFAULT_SPEC as SPEC
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import rng

from . import generic_kernel_refs as G
from .generic_kernel_refs import EPS, MOMENTUM, U32, UB

SR, HALO, L, SLOTS = 64, 4, 60, 16          # csrc/train_geo.h kSR, kHalo, kL; train_args.h kStatSlots
CH = list(SPEC.channels())                   # [4, 128, 192, 224, 96, 256, 96]
KS = [b.kernel_size for b in SPEC.blocks]
RATES = [b.dropout for b in SPEC.blocks]
TAB_ROWS, T_MEAN, T_RSTD, T_S, T_T, T_MDY, T_MDYX = 6, 0, 1, 2, 3, 4, 5
PASS = (1 << 30) + 5                         # the dropout pass the fixtures draw their masks for
OMM = 1.0 - MOMENTUM                         # 1.f - momentum is exact in fp32 and in float64


# ------------------------------------------------------------------------------------------ launch geometry
# Stated once, in csrc/train_geo.h.  The tests learn it by running the stand-alone host program
# tests/train_geo_check.cpp (which also checks the header against brute force, test_train_geo_cpu.py): built
# once per session into a temporary directory, with the wgrad table csrc/build.py would build the kernels with.
def geo_check_exe():
    return G.geo_check_exe("train_geo_check", tuple(d for d in build.EXTRA if d.startswith("-DAPNEAUQ_WG_TABLE=")))


@functools.lru_cache(maxsize=None)
def geo(n, M=1, det=False):
    """The launch geometry of M members x n samples (``--table``): ``tiles``, ``fwd_train_grid``, ``dg_grid``,
    ``head`` (spw, grid) and per block ``fwd`` (pf, grid), ``dgrad`` (persist, grid), ``wgrad`` (cib, cob,
    rtiles, cap, rgs, rt = row tiles per group, grid, J, ...)."""
    r = subprocess.run([geo_check_exe(), "--table", str(n), str(M), str(int(det))], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def wg(l, n, M=1):
    return geo(n, M)["blocks"][l]["wgrad"]


def tiles(n):
    return (n + 1) // 2


# ------------------------------------------------------------------------------------------ layout
def f32(t, on=True):
    return t.float().double() if on else t


def bf(t, on=True):
    return t.bfloat16().double() if on else t


def padded_rows(n):
    return 128 * tiles(n) + 2 * HALO


def place(buf, v):
    """(n, 60, C) into the valid rows of a padded-row buffer (rows, C)."""
    n = v.shape[0]
    buf[HALO: HALO + SR * n].view(n, SR, -1)[:, :L] = v.to(buf.dtype)
    return buf


def take(buf, n):
    """The valid rows (n, 60, C) of a padded-row buffer."""
    return buf[HALO: HALO + SR * n].view(n, SR, -1)[:, :L]


def valid_rows(rows, n):
    """(rows,) bool: the rows holding a time step of a sample < n."""
    r = torch.arange(rows) - HALO
    return (r >= 0) & (r // SR < n) & (r % SR < L)


def encode(mag, drop):
    """bf16 R: |R| = mag, sign bit = dropped (a dropped zero is -0.0, a kept one +0.0)."""
    b = mag.bfloat16()
    return torch.where(drop, -b, b)


def sign_bits(t):
    return t.contiguous().view(torch.int16) < 0


def dsc(l):
    """1 / (1 - p) of block l as the ctx carries it (a float)."""
    return float(np.float32(1.0 / (1.0 - RATES[l])))


def keep_mask(seed, l, n, dev="cpu", pass_id=PASS, woff=0):
    """Block l's keep mask (n, 60, C[l + 1]) as the producer kernel draws it."""
    return rng.keep_mask_torch(rng.stream_key(seed, l, pass_id), woff + torch.arange(n, device=dev), L, CH[l + 1],
                               RATES[l])


# ------------------------------------------------------------------------------------------ BN rows / table
def bn_rows64(st, inv_count, gamma, beta, eps=EPS):
    """Forward rows of the parameter table from the moment slots ``st`` (SLOTS, 2, C) fp64: mean, rstd,
    s = gamma rstd, t = beta - mean s (plus var, E[r^2]); the slots are added in extended precision."""
    dev = st.device
    mean, var, eu2 = (v.to(dev) for v in G.bn_moments64(st.reshape(-1, 2, st.shape[-1]), inv_count))
    rstd = 1.0 / torch.sqrt(var + eps)
    s = gamma.double() * rstd
    return dict(mean=mean, var=var, eu2=eu2, rstd=rstd, s=s, t=beta.double() - mean * s)


def bn_rows_allow(r, gamma, beta, eps=EPS):
    """var: its fp32 rounding and the fp64 cancellation E[r^2] - mean^2 (16 slot additions, the two products
    by inv_count, the square, the difference: < 2^-47 E[r^2]).  mean: one fp32 rounding.  rstd: 4 ulps of
    rsqrtf / the eps addition plus the variance's allowance through d rstd / d var = rstd / (2 (var + eps)).
    s, t: one / two more fp32 roundings, their inputs' allowances carried."""
    a_var = 2.0 ** -23 * r["var"] + 2.0 ** -47 * r["eu2"]
    a_mean = 2.0 ** -23 * r["mean"].abs()
    a_rstd = 2.0 ** -21 * r["rstd"] + 0.5 * r["rstd"] / (r["var"] + eps) * a_var
    a_s = 2.0 ** -23 * r["s"].abs() + gamma.double().abs() * a_rstd
    a_t = 2.0 ** -22 * (beta.double().abs() + (r["mean"] * r["s"]).abs()) + r["mean"].abs() * a_s + r["s"].abs() * a_mean
    return dict(mean=a_mean, var=a_var, rstd=a_rstd, s=a_s, t=a_t)


def slot_mean64(bst, inv_count):
    """Backward rows (mean dY, mean dY xhat) from ``bst`` (SLOTS, 2, C) fp64 -> (rows (2, C), allowance): one
    fp32 rounding of an fp64 sum of 16 slots."""
    b = bst.reshape(-1, 2, bst.shape[-1])
    s = b.detach().cpu().numpy().astype(np.longdouble)
    tot = torch.from_numpy((s.sum(0) * np.longdouble(inv_count)).astype(np.float64)).to(bst.device)
    ab = b.abs().sum(0) * inv_count
    return tot, 2.0 ** -23 * tot.abs() + 2.0 ** -48 * ab


def finalize64(st, bst, inv_count, mmean, mvar, hpart=None):
    """``bn_finalize_kernel`` of one block: moving averages, dgamma = sum dY xhat, dbeta = sum dY and, for the
    head's slots ``hpart`` (SLOTS, C + 2), the dense gradients and the loss -> (refs, allowances)."""
    r = bn_rows64(st, inv_count, torch.ones_like(mmean), torch.zeros_like(mmean))
    a_var = 2.0 ** -23 * r["var"] + 2.0 ** -47 * r["eu2"]
    mm, mv = mmean.double(), mvar.double()
    ref = dict(mmean=mm * MOMENTUM + r["mean"] * OMM, mvar=mv * MOMENTUM + r["var"] * OMM)
    al = dict(mmean=2.0 ** -22 * ((mm * MOMENTUM).abs() + (r["mean"] * OMM).abs()),
              mvar=2.0 ** -22 * ((mv * MOMENTUM).abs() + r["var"] * OMM) + OMM * a_var)
    b = bst.reshape(-1, 2, bst.shape[-1])
    tot = torch.from_numpy(b.detach().cpu().numpy().astype(np.longdouble).sum(0).astype(np.float64)).to(bst.device)
    a_tot = 2.0 ** -23 * tot.abs() + 2.0 ** -48 * b.abs().sum(0)
    ref.update(gbeta=tot[0], ggamma=tot[1])
    al.update(gbeta=a_tot[0], ggamma=a_tot[1])
    if hpart is not None:
        h = hpart.double().reshape(SLOTS, -1)
        ref["head"] = h.sum(0)                       # dense_w grads (C), loss, dense_b grad
        al["head"] = SLOTS * U32 * h.abs().sum(0)    # 16 fp32 additions in slot order
    return ref, al


# ------------------------------------------------------------------------------------------ staging
def stage64(mag, drop, s, t, scale, rnd=True):
    """A = dropout(BN(R)) as the conv kernels stage it: ``bf16(fma(|r|, s', t'))`` with the fp32
    ``s' = s scale``, ``t' = t scale`` (scale = 1 / (1 - p), or 1 with dropout off), 0 where the sign bit is
    set.  -> (A, amb): ``amb`` holds the bf16 ulp of the elements whose float64 value lies within
    ``2^-23 (|r s'| + |t'|)`` of a bf16 rounding boundary (the fp32 fma may round them either way), 0
    elsewhere."""
    s0, t0 = f32(s.double() * scale, rnd), f32(t.double() * scale, rnd)
    v = mag * s0 + t0
    zero = torch.zeros((), dtype=torch.float64, device=mag.device)
    if not rnd:
        return torch.where(drop, zero, v), torch.zeros_like(v)
    a = torch.where(drop, zero, bf(f32(v)))
    av = v.abs()
    _, e = torch.frexp(av)                                   # av = m 2^e, m in [0.5, 1): bf16 ulp 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(av), e - 8)
    dist = (torch.remainder(av / ulp, 1.0) - 0.5).abs() * ulp
    amb = (~drop) & (dist <= 2.0 ** -23 * ((mag * s0).abs() + t0.abs()))
    return a, torch.where(amb, ulp, zero)


# ------------------------------------------------------------------------------------------ forward
def fwd64(a, w, bias, rnd=True, amb=None):
    """relu(conv(A, bf16(w)) + b) of ``fwd_kernel`` -> (ref (n, 60, Cout), allowance, entries widened).
    The allowance is ``conv_allow`` (K + 2 fp32 additions over the absolute terms, one bf16 store); ``amb``
    (from :func:`stage64`) widens exactly the entries reading an ambiguous input."""
    wb = bf(w.double(), rnd)
    ref = G.conv64(a, wb, bias, relu=True, to=G.d64)
    ab = G.conv_abs64(a, wb, bias, to=G.d64)
    allow = G.conv_allow(ref, ab, w.shape[0] * w.shape[1], True)
    nw = 0
    if amb is not None:
        wide = G.conv64(amb, wb.abs(), to=G.d64)
        allow = allow + wide
        nw = int((wide > 0).sum())
    return ref, allow, nw


def fwd_moments(stored_mag, n, grid, l):
    """Moment slots of ``fwd_kernel``: taken from the STORED bf16 tile on the matrix cores (products of two
    bf16 values are exact in fp32), 128 rows per tile accumulated in fp32, one more addition per tile of the
    workgroup and two merges -> (moments64 of the stored tile, allowance)."""
    tpw = -(-tiles(n) // grid)
    ref = G.moments64(stored_mag)
    return ref, (128 + tpw + 2) * U32 * ref      # every term is >= 0: the sums are their own absolute sums


# ------------------------------------------------------------------------------------------ head
def head64(mag, drop, rows, w, b, y, inv_batch, scale, dlog=None):
    """``head_kernel``: A_6 = dropout(BN(R_6)) in fp32 (not rounded to bf16), GAP, Dense, BCE on logits, dlogit,
    dense gradients and the backward sums of block 6.  ``rows``: the fp32 mean / rstd / s / t the kernel
    reads.  ``dlog``: the kernel's own dlogit -- the sums are then held to their own accumulation."""
    w, y = w.double().reshape(-1), y.double()
    keepf = (~drop).double()
    a = (mag * rows["s"] + rows["t"]) * keepf
    aa = ((mag * rows["s"]).abs() + rows["t"].abs()) * keepf
    gap, gapa = a.sum(1) * scale, aa.sum(1) * scale              # (n, C): sums over time, not yet / 60
    z = (gap @ w) / L + b
    za = (gapa @ w.abs()) / L
    p = torch.sigmoid(z)
    d = torch.where(z >= 0, (1.0 - y) - torch.sigmoid(-z), p - y) * inv_batch
    dg = d if dlog is None else dlog.double()
    t1, t2, t3 = torch.clamp(z, min=0), z * y, torch.log1p(torch.exp(-z.abs()))
    dy = keepf * (dg / L)[:, None, None] * (w * scale)
    xh = (mag - rows["mean"]) * rows["rstd"]
    xa = (mag + rows["mean"].abs()) * rows["rstd"]
    return dict(logit=z, logit_terms=za, bias=abs(float(b)), dlog=d, loss=(t1 - t2 + t3).sum(),
                loss_abs=(t1 + t2.abs() + t3).sum(), pmy=(d / inv_batch).abs(),
                gw=(dg[:, None] * gap).sum(0) / L, gw_abs=(dg.abs()[:, None] * gapa).sum(0) / L,
                gb=dg.sum(), gb_abs=dg.abs().sum(),
                bst=torch.stack([dy.sum((0, 1)), (dy * xh).sum((0, 1))]),
                bst_abs=torch.stack([dy.abs().sum((0, 1)), (dy.abs() * xa).sum((0, 1))]))


def head_chain(n, mode, M=1):
    """fp32 additions on the longest chain of one of the head's sums over samples.  'slots': the 4 spw
    samples of a workgroup (LDS atomics), then the workgroups sharing one of 16 slots (the test adds the
    slots in float64); 'atomic': every workgroup onto one address; 'det': fp64 from the per-sample records."""
    spw = geo(n, M)["head"]["spw"]
    nwg = -(-n // (4 * spw))
    return {"slots": 4 * spw + -(-nwg // SLOTS), "atomic": 4 * spw + nwg, "det": 0}[mode]


def head_allow(r, n, inv_batch, mode, M=1):
    """logit: 30 fp32 roundings over the GAP . Dense terms (12 rows and 8 channels per lane, the 6 steps of
    the wave sum, the fma / dropout scale / weight product / division by 60) and one for adding the bias.
    dlogit: 2^-21 relative to ITSELF (expf, the division) plus the logit's error through the sigmoid's
    largest slope on that interval -- a saturated probability must not cancel against its label.
    Sums: their chain (:func:`head_chain`) plus the roundings inside one term, over the absolute terms; the
    loss also carries every sample's logit error times |p - y|."""
    dz = 30 * U32 * r["logit_terms"] + U32 * (r["logit_terms"] + r["bias"])
    za = (r["logit"].abs() - dz).clamp(min=0)
    slope = torch.sigmoid(za) * torch.sigmoid(-za)
    ch = head_chain(n, mode, M)
    spw = geo(n, M)["head"]["spw"]
    return dict(logit=dz, dlog=2.0 ** -21 * r["dlog"].abs() + inv_batch * slope * dz,
                loss=(ch + 6) * U32 * r["loss_abs"] + (r["pmy"] * dz).sum(),
                gw=(ch + 12 + 5 + 4) * U32 * r["gw_abs"], gb=(ch + 1) * U32 * r["gb_abs"],
                bst=(12 + 5 + 4 * spw + 6) * U32 * r["bst_abs"])


# ------------------------------------------------------------------------------------------ dgrad
def dz64(mag, dy, g, mean, rstd, mdy, mdyx):
    """dZ = relu'(r) g (dy - mean(dy) - xhat mean(dy xhat)), g = gamma rstd -> (dz, allowance before the
    store).  The kernel folds it into fma(g, dy, fma(-g q, r, g (q mean - mdy))), q = rstd mdyx: seven fp32
    roundings, each relative to a term of |g| (|dy| + |mdy| + (r + |mean|) rstd |mdyx|)."""
    xh = (mag - mean) * rstd
    pos = mag > 0
    zero = torch.zeros((), dtype=torch.float64, device=mag.device)
    dz = torch.where(pos, g * (dy - mdy - xh * mdyx), zero)
    terms = torch.where(pos, g.abs() * (dy.abs() + mdy.abs() + (mag + mean.abs()) * rstd * mdyx.abs()), zero)
    return dz, 2.0 ** -21 * terms


def head_dy64(drop, dlog, w, scale):
    """dY_6 as dgrad<5> / wgrad<5> recompute it: fp32 (dlogit / 60) (w scale), 0 where dropped."""
    dl = f32(dlog.double() * float(np.float32(1.0 / L)))
    dw = f32(w.double().reshape(-1) * scale)
    return torch.where(drop, torch.zeros((), dtype=torch.float64, device=drop.device), dl[:, None, None] * dw)


def dgrad64(dz_stored, w, keep_prev, scale, rnd=True):
    """dY_{l-1} = mask_{l-1} / (1 - p) conv^T(dZ_l, bf16(w)) -> (ref, allowance): the transposed conv over
    the dZ_l the kernel WROTE (K + 3 fp32 additions over the absolute terms, one bf16 store); dropped
    elements are exactly 0."""
    wt = G.flip_t(bf(w.double(), rnd))
    zero = torch.zeros((), dtype=torch.float64, device=dz_stored.device)
    ref = torch.where(keep_prev, G.conv64(dz_stored, wt, to=G.d64) * scale, zero)
    ab = torch.where(keep_prev, G.conv_abs64(dz_stored, wt, to=G.d64) * scale, zero)
    return ref, (w.shape[0] * w.shape[2] + 3) * U32 * ab + (UB * ref.abs() if rnd else 0)


def bwd_sums64(dy_stored, mag_prev, mean_prev, rstd_prev):
    """bst[l-1] of dgrad<l>: sum dY, sum dY xhat over the dY_{l-1} the kernel STORED -> (sums (2, C),
    allowance): <= 8 rows per lane, 4 steps of the 16-lane sum, then fp64; 3 roundings inside a term of
    sum dY xhat, relative to |dY| (r + |mean|) rstd."""
    xh = (mag_prev - mean_prev) * rstd_prev
    xa = (mag_prev + mean_prev.abs()) * rstd_prev
    ref = torch.stack([dy_stored.sum((0, 1)), (dy_stored * xh).sum((0, 1))])
    ab = torch.stack([dy_stored.abs().sum((0, 1)), (dy_stored.abs() * xa).sum((0, 1))])
    return ref, torch.stack([12 * U32 * ab[0], 15 * U32 * ab[1]])


# ------------------------------------------------------------------------------------------ wgrad
def slots_rows(v, pad):
    """(n, 60, C) -> the rows of the padded layout, ``pad`` zero rows before and after: (64 n + 2 pad, C)."""
    n, _, C = v.shape
    s = torch.zeros(n, SR, C, dtype=v.dtype, device=v.device)
    s[:, :L] = v
    z = torch.zeros(pad, C, dtype=v.dtype, device=v.device)
    return torch.cat([z, s.reshape(n * SR, C), z])


def wgrad64(a, dz, l, n, M=1, amb=None, amb_dz=None):
    """dW_l[tap] = sum_rows A_{l-1}[row + tap - pad] dZ_l[row], db_l = sum_rows dZ_l -> (gw, gb, allowances,
    entries widened).  Chain: the 128 rows of each of a row group's tiles on the matrix cores, then the row
    groups in the reduction's order (at most rgs additions; fp32 atomics without partials: the same count).
    ``amb`` / ``amb_dz``: bf16 ulps of ambiguous elements of A (:func:`stage64`) / of a dZ the kernel formed
    itself (block 1), which widen the entries they enter."""
    k, pad = KS[l], (KS[l] - 1) // 2
    ap, dzp = slots_rows(a, pad), slots_rows(dz, 0)
    R = dzp.shape[0]
    gw, ab = G.wgrad64(ap, dzp, R, k, to=G.d64)
    rgs, rt = wg(l, n, M)["rgs"], wg(l, n, M)["rt"]
    chain = (128 * rt + rgs + 2) * U32
    a_gw, a_gb = chain * ab, chain * dzp.abs().sum(0)
    nw = 0
    for am, other, first in ((amb, dz, True), (amb_dz, a, False)):
        if am is None:
            continue
        x, d = (slots_rows(am, pad), dzp.abs()) if first else (slots_rows(other, pad).abs(), slots_rows(am, 0))
        wide = G.wgrad64(x, d, R, k, to=G.d64)[0]
        a_gw = a_gw + wide
        nw += int((wide > 0).sum())
        if not first:
            a_gb = a_gb + slots_rows(am, 0).sum(0)
    return gw, dzp.sum(0), a_gw, a_gb, nw


# ================================================================================================ fixtures
def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (1 << 31))


def params(seed):
    """fp32 parameters of one model (names of ``models/reference.py``).  Per conv: output channel 0 has
    all-zero weights and bias 0 (R = 0: kept zeros are +0.0 and decode to t, dropped ones -0.0), channel 1 a
    bias of -50 (the ReLU kills everything).  gamma in [0.5, 1.5] with gamma[2] = 0 on every block."""
    g = _gen(11, seed)
    p = {}
    for i in range(1, 7):
        k, ci, co = KS[i - 1], CH[i - 1], CH[i]
        w = torch.randn(k, ci, co, generator=g) / math.sqrt(k * ci)
        b = torch.randn(co, generator=g) * 0.3
        w[:, :, 0] = 0.0
        b[0] = 0.0
        b[1] = -50.0
        gamma = 0.5 + torch.rand(co, generator=g)
        gamma[2] = 0.0
        p[f"conv1d_{i}/kernel"], p[f"conv1d_{i}/bias"] = w, b
        p[f"batchnorm_{i}/gamma"], p[f"batchnorm_{i}/beta"] = gamma, 2 * torch.rand(co, generator=g) - 1
        p[f"batchnorm_{i}/moving_mean"] = torch.randn(co, generator=g)
        p[f"batchnorm_{i}/moving_variance"] = 0.5 + torch.rand(co, generator=g)
    p["output_layer/kernel"] = torch.randn(CH[6], 1, generator=g) / math.sqrt(CH[6])
    p["output_layer/bias"] = torch.full((1,), 0.25)
    return {k: v.float() for k, v in p.items()}


def act_fixture(l, n, seed, dropout=True, tag=0):
    """R_l (n, 60, C[l+1]) as a forward kernel leaves it -> (mag float64 of bf16 values, drop bool): post-ReLU
    magnitudes (about half zeros) at mixed channel scales; channel 0 all zero, channel 1 constant; the mask
    drawn with ``ops/rng.py`` for (seed, l, PASS), nothing dropped with dropout off."""
    C = CH[l + 1]
    g = _gen(12, l, n, seed, tag)
    u = torch.relu(torch.randn(n, L, C, generator=g) + 0.2) * (0.25 + 2 * torch.rand(C, generator=g))
    u[:, :, 0] = 0.0
    u[:, :, 1] = 0.75
    mag = bf(u.double())
    drop = ~keep_mask(seed, l, n) if dropout else torch.zeros(n, L, C, dtype=torch.bool)
    return mag, drop


def grad_fixture(l, n, seed, tag=0):
    """A bf16 gradient (n, 60, C[l+1]) at the scale of a batch-mean loss."""
    g = _gen(13, l, n, seed, tag)
    return bf((torch.randn(n, L, CH[l + 1], generator=g) / max(n, 1)).double())


def moment_slots(mag, nslots=SLOTS):
    """fp64 slots (nslots, 2, C) whose sum is the moments of ``mag`` (n, 60, C): the rows dealt round-robin."""
    r = mag.reshape(-1, mag.shape[-1])
    out = torch.zeros(nslots, 2, r.shape[1], dtype=torch.float64, device=mag.device)
    for s in range(nslots):
        out[s, 0], out[s, 1] = r[s::nslots].sum(0), (r[s::nslots] ** 2).sum(0)
    return out


BN_COUNT = 3840     # 64 samples x 60: not a power of two (a float 1 / 3840 is off by 2^-25.4)


def bn_edge_slots(C, seed):
    """Moment slots (SLOTS, 2, C) of BN_COUNT fp32 samples per channel, written directly: channel 0 all zero,
    1 constant 0.75 (variance exactly 0), 2 the near-constant channel far from zero (mean 100, std 0.01),
    3 mean 5 / std 1e-3, 4 huge variance (scale 3e3), the rest relu(N(0.3, 1)) at mixed scales."""
    g = _gen(14, C, seed)
    u = torch.relu(torch.randn(BN_COUNT, C, generator=g) + 0.3) * (0.25 + 4 * torch.rand(C, generator=g))
    u[:, 0] = 0.0
    u[:, 1] = 0.75
    u[:, 2] = 100.0 + 0.01 * torch.randn(BN_COUNT, generator=g)
    u[:, 3] = 5.0 + 1e-3 * torch.randn(BN_COUNT, generator=g)
    u[:, 4] = 3e3 * torch.randn(BN_COUNT, generator=g).abs()
    return moment_slots(u.float().double()[None].reshape(BN_COUNT // L, L, C))


def table_rows(mag, gamma, beta, n):
    """fp32 table rows (as float64) of a block whose output is ``mag``: what ``tab_write_fwd`` would leave."""
    r = bn_rows64(moment_slots(mag), 1.0 / (n * L), gamma, beta)
    return {k: f32(r[k]) for k in ("mean", "rstd", "s", "t")}


# ================================================================================================ whole step
def step64(p, x, y, seed, rnd=False, pass_id=PASS):
    """The references composed into one training step (every kernel's reference feeding the next) -> dict of
    logits, loss sum, gradients by parameter name and the moving statistics' updates.  With ``rnd=False``
    this is the float64 step exactly."""
    n = x.shape[0]
    ic, ib = 1.0 / (n * L), 1.0 / n
    dev = x.device
    eps, mom = (EPS, MOMENTUM) if rnd else (SPEC.bn_epsilon, SPEC.bn_momentum)   # the kernels take floats
    a = bf(x.double(), rnd)
    mags, drops, rows, acts = [], [], [], [a]
    for l in range(6):
        i = l + 1
        ref, _, _ = fwd64(a, p[f"conv1d_{i}/kernel"], p[f"conv1d_{i}/bias"], rnd)
        mag = bf(ref, rnd)
        drop = ~keep_mask(seed, l, n, dev, pass_id)
        r = bn_rows64(moment_slots(mag), ic, p[f"batchnorm_{i}/gamma"], p[f"batchnorm_{i}/beta"], eps)
        r = {k: f32(v, rnd) for k, v in r.items()}
        mags.append(mag), drops.append(drop), rows.append(r)
        if l < 5:
            a, _ = stage64(mag, drop, r["s"], r["t"], dsc(l) if rnd else 1.0 / (1.0 - RATES[l]), rnd)
            acts.append(a)
    sc = [dsc(l) if rnd else 1.0 / (1.0 - RATES[l]) for l in range(6)]
    h = head64(mags[5], drops[5], rows[5], p["output_layer/kernel"], p["output_layer/bias"].double(), y, ib, sc[5])
    out = {"logits": h["logit"], "loss": h["loss"], "output_layer/kernel": h["gw"], "output_layer/bias": h["gb"]}
    dlog = f32(h["dlog"], rnd)
    dy = head_dy64(drops[5], dlog, p["output_layer/kernel"], sc[5]) if rnd else \
        torch.where(drops[5], torch.zeros((), dtype=torch.float64, device=dev),
                    (dlog / L)[:, None, None] * p["output_layer/kernel"].double().reshape(-1) * sc[5])
    bst = h["bst"]
    for l in range(5, -1, -1):
        i = l + 1
        out[f"batchnorm_{i}/beta"], out[f"batchnorm_{i}/gamma"] = bst[0], bst[1]
        r = rows[l]
        m = f32(bst * ic, rnd)
        dz, _ = dz64(mags[l], dy, r["s"], r["mean"], r["rstd"], m[0], m[1])
        dz = bf(dz, rnd)
        gw, gb, _, _, _ = wgrad64(acts[l], dz, l, n)
        out[f"conv1d_{i}/kernel"], out[f"conv1d_{i}/bias"] = gw, gb
        out[f"batchnorm_{i}/moving_mean"] = p[f"batchnorm_{i}/moving_mean"].double() * mom + r["mean"] * (1 - mom)
        out[f"batchnorm_{i}/moving_variance"] = p[f"batchnorm_{i}/moving_variance"].double() * mom + r["var"] * (1 - mom)
        if l > 0:
            dyp, _ = dgrad64(dz, p[f"conv1d_{i}/kernel"], ~drops[l - 1], sc[l - 1], rnd)
            dy = bf(dyp, rnd)
            bst, _ = bwd_sums64(dy, mags[l - 1], rows[l - 1]["mean"], rows[l - 1]["rstd"])
    return out
