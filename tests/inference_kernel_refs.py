"""Exact-arithmetic probes, float64 references and allowances of the inference kernels: the fused whole-network
kernels (``csrc/fused_forward.hip``, ``csrc/fused_tiled.hip``, ``csrc/fused_tiled_x3.hip``) and the layer-wise
ones (``csrc/generic_conv.hip`` in ``kInfer`` mode, ``generic_head``).  ``test_inference_kernel_refs_cpu.py``
checks this oracle without a GPU and shows what its allowances catch; ``test_inference_kernels_gpu.py`` holds the
kernels to it.

A fused kernel returns only a logit, and after six bf16 blocks with Gaussian weights the roundings cascade: no
tolerance on such a logit can be tight.  The PROBE networks remove the roundings instead.  Inputs, weights, bias
and BN affine lie on a dyadic grid with bounded magnitudes, so every fp32 product, sum and fma a kernel performs
up to a store is exact, in any order of accumulation.  What is left is the ``(__bf16)`` store, which float64
emulates bit for bit (round to nearest even to 8 bits), nothing at all in the fp16x3 kernels while a value fits
hi + lo, and the few fp32 operations of the head.  :func:`forward64` asserts those conditions itself, per block
and sample: a probe that violates one is a broken fixture, never a wider allowance.

The probes go through the public packers only (``pack_blob``, ``pack_blob_x3``, ``generic.pack``):
``ModelSpec.bn_epsilon = 2^-10`` with ``moving_variance = 1 - 2^-10`` makes ``rsqrt`` return 1, so ``gamma = +-2^-j``
or 0 IS the folded scale; dropout rates 0.5 / 0.75 make the ``1 / (1 - rate)`` rows exact.

Allowances, one line per kernel (``U32 = 2^-23`` per fp32 operation, ``UB = 2^-8`` per bf16 store):

* fused logits, GAP heads (``fused_forward``, single-channel bf16 / x3): while ``sum |dw y6| 2^G < 2^24`` the
  GAP x Dense sum S is exact; left are the rounded ``1 / L`` constant, one multiply, one add:
  ``3 U32 |S| / L + U32 |db|``;
* fused logits, pooled nets (L = 1, the GAP is the identity, no ``1 / L``): one add, ``U32 |S| + U32 |db|``;
* where that bound fails: the additions of the longest chain of the kernel's head (``HEAD_CHAIN``) over
  ``sum |dw y6| / L`` instead of the first term;
* probabilities: the logit allowance and ``|z| U32`` (the rounded argument of ``__expf``) through ``p (1 - p)``,
  plus ``4 U32 p + 2^-126`` as for ``x3_head``;
* ``generic_conv`` (kInfer): ``UB |ref| + (K + 2) U32 |s| (|x| conv |w|) + U32 |t'|``, the larger of the pair
  under a pool, 0 where the mask drops;
* ``generic_head``: ``(ceil(L C / 64) + 6 + 2) U32 sum |w y| / L + U32 |b|`` (a lane's strided chain, the wave
  tree, the division and the add).
"""
import functools
import math

import torch
import torch.nn.functional as F

from uncertaintyquantification_sleepapnea_1dcnn_amd.models.spec import BlockSpec, ModelSpec
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import fused, rng

from . import generic_kernel_refs as GK

U32 = 2.0 ** -23
UB = 2.0 ** -8
BN_EPS = 2.0 ** -10
KINDS = ("nopool", "pooled", "single")
FILTERS = (128, 192, 224, 96, 256, 96)
KSIZES = (7, 5, 3, 7, 9, 9)
RATES = (0.5, 0.5, 0.75, 0.5, 0.5, 0.5)
N_NETS = 3                     # probe nets per spec (one member stack); the last one is the zero-path net
# non-zero weights per output channel on the taps that reach a valid row.  The density of block l + 1 decides how
# visible a stored element of block l is in the logit (test_one_grid_unit_is_visible); a pool hides the smaller of
# every pair, so the pooled probes are denser
NNZ = {"nopool": (4, 6, 6, 10, 6, 24), "pooled": (4, 12, 8, 32, 16, 16), "single": (4, 6, 6, 10, 6, 24)}
SEED, PASS_OFF, WIN_OFF = 0x5EED1234ABCD, 5, 11
SCALE_EXPS = (0, 7, -9)        # the same window at 2^0, 2^7, 2^-9 next to each other

# kernel -> (probe kind, arithmetic, samples per workgroup)
KERNELS = {
    "fused_forward": ("nopool", "fused", 2),
    "fused_pooled": ("pooled", "fused", 8),
    "fused_single": ("single", "fused", 4),
    "fused_pooled_x3": ("pooled", "x3", 4),
    "fused_single_x3": ("single", "x3", 2),
}
# fp32 additions on the longest chain of each head, used only where the exact-sum bound fails:
#   fused_forward: product + 3 (a lane's 4 channels) + 4 (row tiles) + 6 (wave tree) + 6 (channel tiles)
#   single-channel nets: product + 3 + 6 (2 row tiles x 3 channel tiles) + 4 (16-lane tree) + 2 (quarters) + 2 (columns)
#   pooled nets (one row per sample): product + 3 + 2 (channel tiles) + 2 (quarters) + 3 (waves)
HEAD_CHAIN = {"fused_forward": 20, "fused_single": 18, "fused_single_x3": 18, "fused_pooled": 11, "fused_pooled_x3": 11}


def ratio(dev, allow):
    """Largest |deviation| / allowance; a non-finite deviation, or a non-zero one under a zero allowance, is inf."""
    dev, allow = dev.abs().reshape(-1).double(), allow.reshape(-1).double()
    inf = torch.full_like(dev, float("inf"))
    r = torch.where(allow > 0, dev / allow.clamp(min=1e-300), torch.where(dev > 0, inf, torch.zeros_like(dev)))
    r = torch.where(torch.isfinite(dev), r, inf)
    return float(r.max())


# ================================================================================================ probes
@functools.lru_cache(maxsize=None)
def probe_spec(kind):
    if kind == "single":
        L, cin, pool = 30, 1, (False,) * 6
    else:
        L, cin, pool = 60, 4, fused.POOLED_PATTERN if kind == "pooled" else (False,) * 6
    blocks = tuple(BlockSpec(f, k, r, bool(pl)) for f, k, r, pl in zip(FILTERS, KSIZES, RATES, pool))
    spec = ModelSpec(L, cin, blocks, bn_epsilon=BN_EPS)
    assert fused.supports(spec) if kind == "nopool" else fused.tiled_net(spec) == (0 if kind == "pooled" else 1)
    return spec


def effective_taps(spec, l):
    """Taps of block ``l`` that reach a valid input row from an output row the block keeps (all of them unless
    the input is shorter than the kernel: pooled blocks 5 and 6)."""
    lin, b = spec.lengths()[l], spec.blocks[l]
    keep = 2 * (lin // 2) if b.pool else lin
    pad = (b.kernel_size - 1) // 2
    return [tap for tap in range(b.kernel_size) if -(keep - 1) <= tap - pad <= lin - 1]


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (1 << 31)
    return torch.Generator().manual_seed(seed)


def _kind_id(kind):
    return KINDS.index(kind)


@functools.lru_cache(maxsize=None)
def probe_params(kind, net):
    """Parameters (fp32, Keras names) of probe net ``net`` of a spec.  Sparse +-1 / +-2 kernels whose non-zero
    rows walk a fixed permutation of the block's k-rows, so that the ``N_NETS`` nets together put a weight on
    every (tap, ci); scale +-1 (block 1) / +-0.5 with negative and zero channels in every block; integer bias,
    shift and dense head.  The last net has bias <= 0 and shift 0 everywhere: an all-zero window stays zero
    through every block."""
    spec = probe_spec(kind)
    ch = spec.channels()
    zero_path = net == N_NETS - 1
    p = {}
    for l, b in enumerate(spec.blocks):
        i, k, cin, cout = l + 1, b.kernel_size, ch[l], b.filters
        g = _gen(_kind_id(kind), l, 17)          # shared by the nets: the permutation they walk
        eff = effective_taps(spec, l)
        rows_eff = torch.tensor([t * cin + c for t in eff for c in range(cin)])
        rows_rest = torch.tensor([t * cin + c for t in range(k) if t not in eff for c in range(cin)], dtype=torch.long)
        rows_eff = rows_eff[torch.randperm(len(rows_eff), generator=g)]
        rows_rest = rows_rest[torch.randperm(len(rows_rest), generator=g)] if len(rows_rest) else rows_rest
        nnz = min(NNZ[kind][l], len(rows_eff))
        nrest = -(-len(rows_rest) // (cout * N_NETS))
        g = _gen(_kind_id(kind), l, net)
        w = torch.zeros(k * cin, cout)
        for co in range(cout):
            base = (net * cout + co) * nnz
            r = rows_eff[(base + torch.arange(nnz)) % len(rows_eff)]
            if nrest:
                base = (net * cout + co) * nrest
                r = torch.cat([r, rows_rest[(base + torch.arange(nrest)) % len(rows_rest)]])
            mag = torch.where(torch.rand(len(r), generator=g) < 0.2, 2.0, 1.0)
            sgn = torch.where(torch.rand(len(r), generator=g) < 0.5, -1.0, 1.0)
            w[r, co] = mag * sgn
        u = torch.rand(cout, generator=g)
        scale = torch.where(u < 0.10, -1.0, torch.where(u < 0.15, 0.0, 1.0)) * (1.0 if l == 0 else 0.5)
        forced = torch.randperm(cout, generator=g)[:2]       # a negative and a zero channel whatever u drew
        scale[forced[0]], scale[forced[1]] = -(1.0 if l == 0 else 0.5), 0.0
        assert ((scale.reshape(-1, 16) != 0).sum(1) >= 8).all(), "every channel tile keeps non-zero channels"
        bias = torch.randint(-2, 1 if zero_path else 3, (cout,), generator=g).float()
        shift = torch.zeros(cout) if zero_path else torch.randint(-1, 2, (cout,), generator=g).float()
        mm = 2.0 * torch.randint(-1, 2, (cout,), generator=g).float()
        p[f"conv1d_{i}/kernel"] = w.reshape(k, cin, cout)
        p[f"conv1d_{i}/bias"] = bias
        p[f"batchnorm_{i}/gamma"] = scale
        p[f"batchnorm_{i}/beta"] = shift + mm * scale
        p[f"batchnorm_{i}/moving_mean"] = mm
        p[f"batchnorm_{i}/moving_variance"] = torch.full((cout,), 1.0 - BN_EPS)
    g = _gen(_kind_id(kind), 6, net)
    # +-2 / +-3 in equal numbers: a dense weight of 0 or +-1 would hide its channel at the size of one grid unit,
    # and a non-zero sum would add the mean of block 6 to every logit (the allowance grows with |S|)
    dw = torch.tensor([2.0, -2.0, 3.0, -3.0]).repeat(ch[6] // 4)
    p["output_layer/kernel"] = dw[torch.randperm(ch[6], generator=g)].reshape(-1, 1)
    p["output_layer/bias"] = torch.randint(-2, 3, (1,), generator=g).float()
    return p


def with_dense_exp(p, e):
    """The net with its dense kernel scaled by 2^e (the probability cases keep |z| <= 8 this way)."""
    q = dict(p)
    q["output_layer/kernel"] = p["output_layer/kernel"] * 2.0 ** e
    return q


def rows_covered(kind):
    """Per block: does every k-row carry a non-zero weight in at least one net?"""
    out = []
    for l in range(6):
        nz = sum((probe_params(kind, m)[f"conv1d_{l + 1}/kernel"] != 0).any(2).reshape(-1).long() for m in range(N_NETS))
        out.append(bool((nz > 0).all()))
    return out


@functools.lru_cache(maxsize=None)
def probe_windows(kind, n):
    """(n, L, Cin) fp32 probe windows: integers in [-4, 4]; windows 0-2 are one window at 2^0, 2^7, 2^-9,
    window 3 is all zero (where n allows)."""
    spec = probe_spec(kind)
    g = _gen(_kind_id(kind), 99)
    x = torch.randint(-4, 5, (max(n, 5), spec.input_length, spec.input_channels), generator=g).float()
    if n >= 3:
        for j, e in enumerate(SCALE_EXPS):
            x[j] = x[0] * 2.0 ** e
    if n >= 4:
        x[3] = 0.0
    return x[:n].contiguous()


# ================================================================================================ reference
def grid_exp(v):
    """Per sample: the smallest G >= 0 with v 2^G integral (v: (n, ...) float64)."""
    n = v.shape[0]
    f = v.reshape(n, -1)
    G = torch.full((n,), -1, dtype=torch.long)
    for e in range(0, 64):
        s = f * 2.0 ** e
        ok = (s == s.round()).all(1) & (G < 0)
        G[ok] = e
        if (G >= 0).all():
            return G
    raise AssertionError("probe values are not dyadic")


def bf16_rne(v):
    """The ``(__bf16)`` store in float64: the value must be an fp32 number (the kernel's register holds it
    exactly), then rounds to nearest even at 8 bits."""
    assert torch.equal(v.float().double(), v), "the value to store is not an fp32 number"
    return v.float().to(torch.bfloat16).double()


def x3_exp(v):
    """Per-sample prescale exponent of the x3 kernels: max |v| 2^e in [2^13, 2^14); 0 for an all-zero sample."""
    m = v.reshape(v.shape[0], -1).abs().amax(1)
    e = 14 - torch.frexp(m)[1].long()
    return torch.where(m > 0, e, torch.zeros_like(e))


def assert_x3_fits(v, what):
    """The sample's values fit hi + lo (two fp16 numbers) at the sample's own exponent, lo normal or zero."""
    e = x3_exp(v).reshape(-1, *([1] * (v.dim() - 1)))
    s = torch.ldexp(v, e)
    hi = s.float().to(torch.float16)
    lo = (s - hi.double()).float().to(torch.float16)
    assert torch.equal(hi.double() + lo.double(), s), f"{what}: a value does not fit hi + lo"
    assert bool(((lo == 0) | (lo.double().abs() >= 2.0 ** -14)).all()), f"{what}: a subnormal lo"


def _pad_conv(h, w, fault=None):
    """'same' conv in float64 over explicit padding rows.  h (n, L, Cin), w (k, Cin, Cout) -> (n, L, Cout)."""
    k, L = w.shape[0], h.shape[1]
    pad = (k - 1) // 2
    hp = F.pad(h.transpose(1, 2), (pad, pad))
    if pad and fault == "halo_one":        # the first row behind every sample reads 1
        hp[:, :, pad + L] = 1.0
    if pad and fault == "leak_prev":       # t = -1 of sample s is the last row of sample s - 1
        hp[1:, :, pad - 1] = h[:-1, L - 1, :]
    y = F.conv1d(hp, w.permute(2, 1, 0)).transpose(1, 2).contiguous()
    if L >= 2 and fault == "tap_first":    # the centre tap of row 0 reads row 1
        y[:, 0] += (h[:, 1] - h[:, 0]) @ w[pad]
    if L >= 2 and fault == "tap_last":     # the centre tap of row L-1 reads row L-2
        y[:, L - 1] += (h[:, L - 2] - h[:, L - 1]) @ w[pad]
    return y


class Result:
    """acts: the six stored activations (n, Lout, C) float64; logit (n,); S, Sabs: the GAP x Dense sum and its
    absolute terms; head_exact (n,): the exact-sum bound holds; db; margin: the largest share of an exactness
    bound that any block and sample uses (only after ``check``)."""


def forward64(kind, p, x, passes, windows, *, arith, dropout=False, seed=SEED, check=True, fault=None,
              fault_block=1, start=0, neighbour=None):
    """float64 forward of probe net ``p`` on samples ``x`` (n, L, Cin) with global (pass, window) ids.

    ``arith``: "fused" (bf16 store between blocks, block 6 stays fp32), "layer" (bf16 store after every block:
    the layer-wise path) or "x3" (no store rounds).  ``check`` asserts the exactness conditions.  ``start``:
    ``x`` is the stored activation of block ``start`` (0: the input).  ``fault``: one deliberate mistake, applied
    in block ``fault_block`` (0-based) -- the mutations of the CPU tests."""
    spec = probe_spec(kind)
    ch = spec.channels()
    h = x.double()
    n = h.shape[0]
    passes, windows = torch.as_tensor(passes).long(), torch.as_tensor(windows).long()
    if check and start == 0:
        if arith == "x3":
            assert_x3_fits(h, "input")
        else:
            assert torch.equal(h.float().to(torch.bfloat16).double(), h), "the input is not bf16"
    out = Result()
    out.acts = []
    for l in range(start, 6):
        b, i = spec.blocks[l], l + 1
        ft = fault if l == fault_block else None
        w = p[f"conv1d_{i}/kernel"].double()
        bias = p[f"conv1d_{i}/bias"].double()
        scale, shift = (v.double() for v in fused.bn_affine(spec, p, i))
        tq = (p[f"conv1d_{i}/bias"].float() * fused.bn_affine(spec, p, i)[0] + fused.bn_affine(spec, p, i)[1]).double()
        acc = _pad_conv(h, w, ft)
        if ft == "pad_lanes" and l == 0:   # the k-lanes behind K = k Cin carry weight 1 and read on: row t + 4
            nx = F.pad(h, (0, 0, 0, 4))[:, 4:4 + h.shape[1]]
            acc = acc + nx.sum(2, keepdim=True)
        if ft == "x3_neighbour" and neighbour is not None:   # acc unscaled by the neighbouring sample's exponent
            acc = torch.ldexp(acc, (neighbour[0] - neighbour[1]).reshape(-1, 1, 1))
        if check:
            G = grid_exp(h) + int(grid_exp(w.reshape(1, -1))[0])
            sabs = _pad_conv(h.abs(), w.abs()).reshape(n, -1).amax(1)
            lim = 2.0 ** 23 if arith == "x3" else 2.0 ** 24
            assert bool((sabs * 2.0 ** G.double() < lim).all()), f"block {i}: an accumulator is not exact"
            out.margin = max(getattr(out, "margin", 0.0), float((sabs * 2.0 ** G.double() / lim).max()))
            assert torch.equal(tq, bias * scale + shift), f"block {i}: the folded shift rounds"
            Ga = G + int(grid_exp(scale.reshape(1, -1))[0])
            amag = ((acc * scale).abs() + tq.abs()).reshape(n, -1).amax(1) / (1.0 - b.dropout)
            assert bool((amag * 2.0 ** Ga.double() < 2.0 ** 24).all()), f"block {i}: the affine is not exact"
            out.margin = max(out.margin, float((amag * 2.0 ** Ga.double() / 2.0 ** 24).max()))
        if ft == "pool_before_affine":
            u = torch.relu(acc + bias)
            u = torch.maximum(u[:, 0:2 * (u.shape[1] // 2):2], u[:, 1:2 * (u.shape[1] // 2):2])
            y = u * scale + shift
        else:
            y = torch.relu(acc + bias) * scale + shift
            if b.pool:
                lo = y.shape[1] // 2
                if ft == "pool_shift":     # the pool over (t + 1, t + 2)
                    yp = F.pad(y, (0, 0, 0, 2))
                    y = torch.maximum(yp[:, 1:2 * lo + 1:2], yp[:, 2:2 * lo + 2:2])
                else:
                    y = torch.maximum(y[:, 0:2 * lo:2], y[:, 1:2 * lo:2])
        if ft == "tile_swap":              # channel tiles 0 and 1 change places
            y = torch.cat([y[..., 16:32], y[..., 0:16], y[..., 32:]], -1)
        if dropout and b.dropout > 0:
            lay = l + 1 if ft == "mask_layer" else l
            ps = passes + 1 if ft == "mask_pass" else passes
            ws = windows
            if ft == "slot_key":           # the key of slot 1 for slot 0 of every sample pair
                idx = torch.arange(n)
                src = torch.where((idx % 2 == 0) & (idx + 1 < n), idx + 1, idx)
                ps, ws = ps[src], ws[src]
            lm = y.shape[1] * 2 if (ft == "mask_unpooled" and b.pool) else y.shape[1]
            keep = torch.empty(n, lm, ch[i], dtype=torch.bool)
            for pv in ps.unique().tolist():
                sel = ps == pv
                keep[sel] = rng.keep_mask_torch(rng.stream_key(seed, lay, pv), ws[sel], lm, ch[i], b.dropout)
            if lm != y.shape[1]:
                keep = keep[:, 0::2]
            y = torch.where(keep, y * (1.0 / (1.0 - b.dropout)), torch.zeros((), dtype=y.dtype))
        if arith == "x3":
            if check and l < 5:
                assert_x3_fits(y, f"block {i}")
        elif arith == "layer" or l < 5:
            y = bf16_rne(y) if check else y.float().to(torch.bfloat16).double()
        out.acts.append(y)
        h = y
    dw = p["output_layer/kernel"].double().reshape(-1)
    db = p["output_layer/bias"].double().reshape(-1)[0]
    L = h.shape[1]
    out.S = (h * dw).sum((1, 2))
    out.Sabs = (h * dw).abs().sum((1, 2))
    out.L, out.db = L, db
    inv = 1.0 / 64.0 if (fault == "gap64" and L > 1) else 1.0 / L
    out.logit = out.S * inv + db
    G6 = grid_exp(h) + int(grid_exp(dw.reshape(1, -1))[0])
    out.head_exact = out.Sabs * 2.0 ** G6.double() < 2.0 ** 24
    return out


def head_allow(kernel, r):
    """Allowance of a fused kernel's logit (see the module text)."""
    first = 1.0 if r.L == 1 else 3.0
    exact = first * U32 * r.S.abs() / r.L
    chain = HEAD_CHAIN[kernel] * U32 * r.Sabs / r.L
    return torch.where(r.head_exact, exact, chain + exact) + U32 * abs(float(r.db))


def prob_ref(z, a_z):
    """-> (probability, its allowance) of a head that returns ``1 / (1 + __expf(-z))``."""
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    return p, (a_z + z.abs() * U32) * p * q + 4 * U32 * p + 2.0 ** -126


def launch_samples(n_win, n_pass, dropout):
    """(window index, global pass id, global window id) of every sample of a launch, pass-major -- the order
    of the kernels' (members, n_pass, n_win) output.  Without dropout every pass is the same: one pass."""
    np_ = n_pass if dropout else 1
    widx = torch.arange(n_win).repeat(np_)
    passes = torch.arange(np_).repeat_interleave(n_win) + PASS_OFF
    return widx, passes, widx + WIN_OFF


@functools.lru_cache(maxsize=None)
def probe_reference(kind, arith, n_win, n_pass, dropout, net, dense_exp=0):
    """The reference of one launch of the probe windows for one member (cached: computed once per session)."""
    x = probe_windows(kind, n_win)
    widx, passes, wins = launch_samples(n_win, n_pass, dropout)
    p = with_dense_exp(probe_params(kind, net), dense_exp)
    return forward64(kind, p, x[widx], passes, wins, arith=arith, dropout=dropout)


def prob_dense_exp(kind, arith, n_win, net):
    """The power of two that brings every logit of the launch to |z| <= 8."""
    r = probe_reference(kind, arith, n_win, 1, False, net)
    m = float((r.S.abs() / r.L).max())
    return 0 if m <= 6.0 else -int(math.ceil(math.log2(m / 6.0)))


# ================================================================================================ generic_conv
CONV_CINS = (32, 320, 1, 4, 12)     # conv_lds_kernel, conv_block_kernel<true>, conv_block_kernel<false> x 3
CONV_KS = (1, 3, 9)
_CONV_SHAPES = ((7, True), (30, True), (30, False), (7, False))    # (L, pool)
_CONV_COUTS = (4, 20, 96, 132)
_CONV_ROWS = (8, 120, 136)          # n * Lp


def conv_cases():
    """The generic_conv cases: every (cin, k) with L / pool, cout, rows and dropout cycled through."""
    cases, j = [], 0
    for cin in CONV_CINS:
        for k in CONV_KS:
            L, pool = _CONV_SHAPES[j % 4]
            Lp = (L + 1) // 2 * 2 if pool else L
            cout = _CONV_COUTS[(j + j // 4) % 4]
            rows = _CONV_ROWS[j % 3]
            drop = j % 2 == 1
            n_win = 3 if j % 4 == 1 else 1
            n = max(1, round(rows / Lp))
            if drop:
                n = max(n_win, n // n_win * n_win)
            cases.append(dict(cin=cin, k=k, L=L, pool=pool, cout=cout, n=n, n_win=n_win if drop else n, drop=drop,
                              rate=(0.5, 0.3)[j % 2 == 1 and j % 3 == 0], layer=j % 6))
            j += 1
    # the corners the cycle leaves out: a one-sample 8-row launch, 136 rows with a second column and a mask
    cases.append(dict(cin=32, k=3, L=7, pool=True, cout=132, n=1, n_win=1, drop=True, rate=0.5, layer=2))
    cases.append(dict(cin=4, k=9, L=7, pool=True, cout=132, n=18, n_win=3, drop=True, rate=0.3, layer=4))
    cases.append(dict(cin=320, k=3, L=30, pool=True, cout=96, n=4, n_win=1, drop=True, rate=0.5, layer=0))
    return cases


def conv_kernel_of(c):
    """Which kernel ``launch_generic_conv`` picks: the plan of csrc/generic_geo.h (inference: in_rs = L)."""
    L, cpad = c.get("L", 30), (c.get("cout", 16) + 15) // 16 * 16
    kind = GK.geo_table("conv", GK.BF16, GK.INFER, c.get("n", 1), L, c["cin"], cpad, c["k"], int(c.get("pool", False)), L)["kind"]
    return {"staged": "conv_lds_kernel", "vec": "conv_block_kernel<true>", "elem": "conv_block_kernel<false>"}[kind]


def conv_fixture(c, idx):
    """Random bf16 input, bf16 kernel, bias / scale (both signs and 0) / shift; the packed fragments and the
    (8, Cout_pad) epilogue rows as ``generic.pack`` builds them."""
    g = _gen(7001, idx)
    cin, k, cout = c["cin"], c["k"], c["cout"]
    cpad = (cout + 15) // 16 * 16
    x = torch.randn(c["n"], c["L"], cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(k, cin, cout, generator=g) / math.sqrt(k * cin)).to(torch.bfloat16)
    bias = torch.randn(cout, generator=g) * 0.3
    scale = torch.randn(cout, generator=g)
    scale[torch.rand(cout, generator=g) < 0.15] = 0.0
    scale[0], scale[1], scale[2] = -1.25, 0.0, 0.75
    shift = torch.randn(cout, generator=g) * 0.2
    pad = lambda v: F.pad(v.float(), (0, cpad - cout))  # noqa: E731
    epi = fused.epilogue_constants(pad(bias), pad(scale), pad(shift))
    epi = torch.cat([epi, epi * (1.0 / (1.0 - c["rate"]))]).contiguous()
    fr = fused.pack_conv_fragments(F.pad(w.float(), (0, cpad - cout)))
    return dict(x=x, w=w, epi=epi, fr=fr, cpad=cpad)


def conv_ref(c, fx, *, fault=None):
    """``generic_conv`` (kInfer) in float64 on the kernel's own inputs -> (ref, allowance, keep mask or None),
    each (n, Lout, Cout)."""
    cout, cpad, K = c["cout"], fx["cpad"], c["k"] * c["cin"]
    x, w = fx["x"].double(), fx["w"].double()
    rows = fx["epi"].double()[4:8] if c["drop"] else fx["epi"].double()[0:4]
    s, tq, lo, hi = (rows[j, :cout] for j in range(4))
    acc, aabs = _pad_conv(x, w), _pad_conv(x.abs(), w.abs())
    y = torch.minimum(torch.maximum(acc * s + tq, lo), hi)
    allow = UB * y.abs() + (K + 2) * U32 * s.abs() * aabs + U32 * tq.abs()
    if c["pool"]:
        lo2 = y.shape[1] // 2
        y = torch.maximum(y[:, 0:2 * lo2:2], y[:, 1:2 * lo2:2])
        allow = torch.maximum(allow[:, 0:2 * lo2:2], allow[:, 1:2 * lo2:2])
    keep = None
    if c["drop"]:
        n, nw = c["n"], c["n_win"]
        idx = torch.arange(n)
        ps, ws = idx // nw, idx % nw
        if fault == "win_is_pass":         # n / n_win taken as the window
            ps, ws = ws, ps
        keep = torch.empty(n, y.shape[1], cout, dtype=torch.bool)
        for pv in ps.unique().tolist():
            sel = ps == pv
            keep[sel] = rng.keep_mask_torch(rng.stream_key(SEED, c["layer"], PASS_OFF + pv), WIN_OFF + ws[sel],
                                            y.shape[1], cout, c["rate"])
        y = torch.where(keep, y, torch.zeros((), dtype=y.dtype))
        allow = torch.where(keep, allow, torch.zeros((), dtype=y.dtype))
    return y, allow, keep


# ================================================================================================ generic_head
HEAD_SHAPES = ((1, 96), (7, 20), (60, 96), (30, 256))
HEAD_NS = (1, 4, 5)


def head_fixture(L, C, n, big):
    """bf16 activations, fp32 dense weights; ``big``: sample 0 sits at a logit of about +30, the last at -30."""
    g = _gen(7002, L, C, n, int(big))
    y = torch.randn(n, L, C, generator=g).to(torch.bfloat16)
    w = torch.randn(C, generator=g) / math.sqrt(C)
    b = float(torch.randn((), generator=g))
    if big:
        y[0] = (30.0 * w.sign() / w.abs().sum()).to(torch.bfloat16).expand(L, C)
        y[n - 1] = -y[0] if n > 1 else y[0]
    return y, w.contiguous(), b


def generic_head_ref(y, w, b):
    """``head_kernel`` in float64 -> (logit, its allowance, probability, its allowance)."""
    n, L, C = y.shape
    yd, wd = y.double(), w.double()
    bd = float(torch.tensor(b, dtype=torch.float32))     # the kernel takes b as float
    z = (yd * wd).sum((1, 2)) / L + bd
    terms = (yd * wd).abs().sum((1, 2)) / L
    a_z = (-(-L * C // 64) + 6 + 2) * U32 * terms + U32 * abs(bd)
    p, a_p = prob_ref(z, a_z)
    return z, a_z, p, a_p
