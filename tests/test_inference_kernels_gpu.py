"""The inference kernels held to the float64 references of ``tests/inference_kernel_refs.py``:

(a) ``generic_conv`` in ``kInfer`` mode (the three kernels its launcher picks between) and ``generic_head``, one
    launch each on random bf16 inputs, every output element under a derived allowance, mask zeros bitwise;
(b) the five fused whole-network kernels on the exact-arithmetic probe networks: logits to the head allowance
    (only the head's few fp32 operations are inexact there), with and without dropout, odd sample counts that
    leave a workgroup straddling two passes, a member stack, an all-zero window, one window at three scales,
    and a window moved between slots (bitwise);
(c) the layer-wise path on the probes: every block's stored activation bitwise, the logit to the
    ``generic_head`` allowance.

Every one of these ops allocates its own output, so there is no buffer to put between sentinel guards: the tests
check the shape and every element instead.  The allowances are derived in the reference module; ``tests/test_inference_kernel_refs_cpu.py`` shows what they
catch.  Each test prints its largest |err| / allowance before it asserts (``profiles/inference_kernel_pins.md``)."""
import functools

import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, fused, generic

from . import inference_kernel_refs as R

pytestmark = pytest.mark.gpu

N_PASS = 3


def _dev():
    return torch.device("cuda")


# ================================================================================================ (a) generic_conv
@pytest.mark.parametrize("idx", range(len(R.conv_cases())))
def test_generic_conv_infer(idx):
    _ext.require()
    c = R.conv_cases()[idx]
    fx = R.conv_fixture(c, idx)
    want, allow, keep = R.conv_ref(c, fx)
    dev = _dev()
    thr = fused.rng.dropout_threshold(c["rate"])
    got = _ext.ops().generic_conv(fx["x"].to(dev), fx["fr"].to(dev), fx["epi"].to(dev), c["cout"], c["k"], c["pool"],
                                  c["drop"], thr, c["layer"], c["n_win"], R.PASS_OFF, R.WIN_OFF, R.SEED & ((1 << 63) - 1))
    torch.cuda.synchronize()
    lout = c["L"] // 2 if c["pool"] else c["L"]
    assert got.shape == (c["n"], lout, c["cout"]) and got.dtype == torch.bfloat16
    got = got.cpu()
    r = R.ratio(got.double() - want, allow)
    tag = f"generic_conv[{R.conv_kernel_of(c)}] case {idx} {c}"
    print(f"{tag}: |err| / allowance {r:.3f}")
    if keep is not None:
        dropped = got[~keep]
        assert 0.1 < float((~keep).double().mean()) < 0.9
        assert not dropped.view(torch.int16).any(), f"{tag}: a dropped entry is not +0"
    assert r <= 1.0, tag


# ================================================================================================ (a) generic_head
@pytest.mark.parametrize("n", R.HEAD_NS)
@pytest.mark.parametrize("shape", R.HEAD_SHAPES)
def test_generic_head(shape, n):
    """Logits and probabilities, ordinary and at a logit of +-30.  The inference heads keep the plain
    ``1 / (1 + __expf(-z))``: at z = -30 it returns exp(-30) to the relative allowance, at z = +30 it returns 1."""
    _ext.require()
    L, C = shape
    o, dev = _ext.ops(), _dev()
    for big in (False, True):
        y, w, b = R.head_fixture(L, C, n, big)
        z, a_z, p, a_p = R.generic_head_ref(y, w, b)
        gz = o.generic_head(y.to(dev), w.to(dev), b, True).cpu().double()
        gp = o.generic_head(y.to(dev), w.to(dev), b, False).cpu().double()
        assert gz.shape == (n,) and gp.shape == (n,)
        rz, rp = R.ratio(gz - z, a_z), R.ratio(gp - p, a_p)
        print(f"generic_head L {L} C {C} n {n} big {big}: logit {rz:.3f}, probability {rp:.3f} (|err| / allowance)")
        if big:
            assert float(z[0]) > 25 and (n == 1 or float(z[n - 1]) < -25)
            assert float(gp[0]) == 1.0 or abs(float(gp[0]) - 1.0) <= 2.0 ** -23
        assert rz <= 1.0 and rp <= 1.0


# ================================================================================================ (b) fused kernels
def _launch(kernel, x, blobs, n_pass, dropout, logits, window_offset=R.WIN_OFF):
    """One launch of a fused kernel -> (members, n_pass, n_win) fp32 on the CPU."""
    kind, arith, _ = R.KERNELS[kernel]
    spec, o, dev = R.probe_spec(kind), _ext.ops(), _dev()
    thr, dsc = fused.dropout_tables(spec)
    s63 = R.SEED & ((1 << 63) - 1)
    if arith == "x3":
        y = o.fused_tiled_x3_forward(x.float().to(dev).contiguous(), blobs, fused.tiled_net(spec), n_pass, window_offset,
                                     R.PASS_OFF, s63, dropout, logits, thr)
    else:
        xb = x.to(torch.bfloat16).to(dev).contiguous()
        if kernel == "fused_forward":
            y = o.fused_forward(xb, blobs, n_pass, window_offset, R.PASS_OFF, s63, dropout, logits, thr, dsc, 0)
        else:
            fn = o.fused_pooled_forward if kernel == "fused_pooled" else o.fused_single_forward
            y = fn(xb, blobs, n_pass, window_offset, R.PASS_OFF, s63, dropout, logits, thr, dsc)
    torch.cuda.synchronize()
    return y.cpu()


@functools.lru_cache(maxsize=None)
def _blobs(kernel, dense_exps=None):
    kind, arith, _ = R.KERNELS[kernel]
    spec = R.probe_spec(kind)
    pack = fused.pack_blob_x3 if arith == "x3" else fused.pack_blob
    nets = [R.with_dense_exp(R.probe_params(kind, m), 0 if dense_exps is None else dense_exps[m]) for m in range(R.N_NETS)]
    return torch.stack([pack(spec, p) for p in nets]).to(_dev())


def _check(kernel, got, refs, what, allow_of, value_of):
    """got (members, n_pass, n_win) against the per-member references; -> the largest |err| / allowance."""
    worst = 0.0
    for m, r in enumerate(refs):
        want, allow = value_of(r), allow_of(r)
        n_win = got.shape[2]
        g = got[m].double().reshape(-1)
        if want.numel() != g.numel():          # without dropout the reference holds one pass
            want, allow = want.repeat(got.shape[1]), allow.repeat(got.shape[1])
        rat = (g - want).abs() / allow.clamp(min=1e-300)
        j = int(rat.argmax())
        worst = max(worst, float(rat[j]))
        assert bool(torch.isfinite(g).all()) and float(rat[j]) <= 1.0, (
            f"{kernel} {what}: member {m} pass {j // n_win} window {j % n_win}: reference {float(want[j])!r} "
            f"got {float(g[j])!r}, |err| / allowance {float(rat[j]):.3f}")
    return worst


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_fused_logits(kernel, full, dropout):
    """n = 1, and n = 2 NS + 1 windows x 3 passes: odd, so a workgroup holds the last window of one pass and
    the first of the next; the windows hold one window at 2^0, 2^7, 2^-9 and the all-zero window (all-zero
    block outputs on the last member's path)."""
    _ext.require()
    kind, arith, ns = R.KERNELS[kernel]
    n_win, n_pass = (2 * ns + 1, N_PASS) if full else (1, 1)
    x = R.probe_windows(kind, n_win)
    got = _launch(kernel, x, _blobs(kernel), n_pass, dropout, True)
    assert got.shape == (R.N_NETS, n_pass, n_win)
    refs = [R.probe_reference(kind, arith, n_win, n_pass, dropout, m) for m in range(R.N_NETS)]
    worst = _check(kernel, got, refs, f"logits n_win {n_win} n_pass {n_pass} dropout {dropout}",
                   lambda r: R.head_allow(kernel, r), lambda r: r.logit)
    print(f"{kernel} n_win {n_win} n_pass {n_pass} dropout {dropout}: logits, |err| / allowance {worst:.3f}")
    if full and not dropout:
        assert float(got[R.N_NETS - 1, 0, 3]) == float(refs[-1].db), "the all-zero window on the zero path"


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_fused_probabilities(kernel, dropout):
    """The dense kernels scaled by a power of two so that |z| <= 8 (without dropout; the masks double it)."""
    _ext.require()
    kind, arith, ns = R.KERNELS[kernel]
    n_win = 2 * ns + 1
    exps = tuple(R.prob_dense_exp(kind, arith, n_win, m) - (2 if dropout else 0) for m in range(R.N_NETS))
    x = R.probe_windows(kind, n_win)
    got = _launch(kernel, x, _blobs(kernel, exps), N_PASS, dropout, False)
    refs = [R.probe_reference(kind, arith, n_win, N_PASS, dropout, m, exps[m]) for m in range(R.N_NETS)]
    inside = [bool((r.logit.abs() <= 8).all()) for r in refs]
    assert dropout or all(inside)
    worst = _check(kernel, got, refs, f"probabilities dropout {dropout}",
                   lambda r: R.prob_ref(r.logit, R.head_allow(kernel, r))[1],
                   lambda r: R.prob_ref(r.logit, R.head_allow(kernel, r))[0])
    print(f"{kernel} dropout {dropout}: probabilities, |err| / allowance {worst:.3f}")


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("kernel", list(R.KERNELS))
def test_fused_slot_invariance(kernel, dropout):
    """One window in slot 0 of one launch and in the last slot of a workgroup of another, under the same global
    window id: bitwise the same logit for every member."""
    _ext.require()
    kind, _, ns = R.KERNELS[kernel]
    x = R.probe_windows(kind, 2 * ns + 1)
    w = x[4:5]
    first = torch.cat([w, x[:ns - 1]])                    # slot 0
    last = torch.cat([x[:ns - 1], w])                     # slot ns - 1
    a = _launch(kernel, first, _blobs(kernel), 1, dropout, True, window_offset=R.WIN_OFF)
    b = _launch(kernel, last, _blobs(kernel), 1, dropout, True, window_offset=R.WIN_OFF - (ns - 1))
    assert torch.equal(a[:, 0, 0].view(torch.int32), b[:, 0, ns - 1].view(torch.int32)), (kernel, a[:, 0, 0], b[:, 0, ns - 1])


# ================================================================================================ (c) layer-wise
@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_layerwise_blocks_bitwise(kind, dropout):
    """``generic_conv`` block by block as ``generic._forward_chunk`` launches it, on the probes: the bf16 store is
    exact or exactly emulated, so every block's stored activation equals the reference's bitwise; the logit of
    ``_forward_chunk`` itself is held to the ``generic_head`` allowance."""
    _ext.require()
    spec, o, dev = R.probe_spec(kind), _ext.ops(), _dev()
    n_win = 5
    x = R.probe_windows(kind, n_win)
    widx, passes, wins = R.launch_samples(n_win, N_PASS, dropout)
    xb = x[widx].to(torch.bfloat16).to(dev).contiguous()
    thr, _ = fused.dropout_tables(spec)
    s63 = R.SEED & ((1 << 63) - 1)
    worst = 0.0
    for m in range(R.N_NETS):
        p = R.probe_params(kind, m)
        packed = generic.pack(spec, {k: v.to(dev) for k, v in p.items()})
        ref = R.probe_reference(kind, "layer", n_win, N_PASS, dropout, m)
        h = xb
        for l, (b, (fr, epi)) in enumerate(zip(spec.blocks, packed["blocks"])):
            h = o.generic_conv(h, fr, epi, b.filters, b.kernel_size, bool(b.pool), dropout, int(thr[l]), l, n_win,
                               R.PASS_OFF, R.WIN_OFF, s63)
            got = h.cpu().double()
            assert got.shape == ref.acts[l].shape
            bad = got != ref.acts[l]
            assert not bad.any(), (f"{kind} member {m} block {l + 1} dropout {dropout}: {int(bad.sum())} stored values "
                                   f"differ, first at {bad.nonzero()[0].tolist()}: reference "
                                   f"{float(ref.acts[l][bad][0])!r} got {float(got[bad][0])!r}")
        z = generic._forward_chunk(packed, spec, xb, n_win, dropout, R.SEED, R.PASS_OFF, R.WIN_OFF, True).cpu().double()
        y6 = ref.acts[5]
        _, a_z, _, _ = R.generic_head_ref(y6, p["output_layer/kernel"].reshape(-1), float(p["output_layer/bias"][0]))
        rz = R.ratio(z - ref.logit, a_z)
        worst = max(worst, rz)
        assert rz <= 1.0, f"{kind} member {m} dropout {dropout}: layer-wise logit, |err| / allowance {rz:.3f}"
    print(f"layer-wise {kind} dropout {dropout}: every block bitwise; logit |err| / allowance {worst:.3f}")
