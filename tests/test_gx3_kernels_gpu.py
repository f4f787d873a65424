"""Every kernel of ``csrc/gx3_conv.hip`` (the fp16x3 layer-wise path of ``train_precision="fp32"`` training and
of fp32 inference for every architecture without a fused kernel) launched alone through
``torch.ops.apneauq.gx3_*`` and held to ``tests/gx3_kernel_refs.py``, in the padded row layout of
``ops/generic_train.py`` (in_rs = L + 2 p, in_off = 2 p forward / p dgrad, pad rows ZERO: this binding's
contract), outputs followed by sentinel rows:

* exact-arithmetic probes: inputs whose halves, products and partial sums are exact in fp32 in any order --
  forward, dgrad and wgrad must equal the arithmetic model bit for bit (a dropped lo hi / hi lo MFMA, a shifted
  tap, swapped channel tiles, a wrong fragment step);
* random cases per entry against the model (fp32 accumulation allowance) and against float64 (+ the split
  allowance), on the smallest shape that reaches each launcher path, with the BN moment slots of both modes;
* mixed magnitudes in one workgroup (what one scale per launch cannot see: a power-of-two prescale commutes
  with the fp16 rounding): per-entry allowances, bitwise scale equivariance, bitwise neighbour independence;
* ``gx3_pack`` bitwise, ``gx3_amax`` at its edges, ``gx3_wgrad`` on its own, and the bindings' rejections.

``test_gx3_kernel_refs_cpu.py`` shows each allowance to be >= 10 times smaller than the mistakes named there.
Each test prints its largest |err| / allowance (none may exceed 1) and the differing entries of its bitwise
tiers (0)."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext

from . import generic_kernel_refs as G
from . import gx3_kernel_refs as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 512.0


def _hold(name, got, ref, allow):
    r = X.ratio(got.detach().double().cpu().reshape(ref.shape) - ref, allow.expand(ref.shape))
    print(f"[ratio] {name}: {r:.4f}")
    assert r <= 1.0, (name, r)
    return r


def _bitwise(name, got, ref):
    """Bit-for-bit: ``got`` (fp32, device or CPU) against ``ref`` (fp32 or float64 values)."""
    g = got.detach().cpu().double().reshape(ref.shape)
    bad = int((g != ref.detach().cpu().double()).sum())
    print(f"[bitwise] {name}: {bad} of {g.numel()} entries differ")
    assert bad == 0, (name, bad)


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _word(v):
    return torch.tensor([X.bits(v)], dtype=torch.int32, device=DEV)


def _as_float(word):
    return float(word.view(torch.float32).item())


def _pack(o, w, dgrad=True):
    k, cin, cout = w.shape
    fwd = torch.empty(X.frag_numel(k, cin, cout), dtype=torch.float16, device=DEV)
    dgr = torch.empty(X.frag_numel(k, cout, cin) if dgrad else 0, dtype=torch.float16, device=DEV)
    wsc = torch.zeros(1, device=DEV)
    o.gx3_pack([_dev(w)], [fwd], [dgr], [wsc], [k], [cin], [cout], torch.empty(16, device=DEV))
    return fwd, dgr, wsc


def _forward(o, xin, fwd, wsc, b, case, det, slots=16, amax=None):
    """Mode 1 -> (y with 4 sentinel rows, slot table, amax word)."""
    cin, L, k, cout, n = case
    p = (k - 1) // 2
    y = torch.full((n * L + 4, cout), SENT, device=DEV)
    st = torch.zeros(slots * 2 * cout, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV) if amax is None else amax
    o.gx3_conv(xin, fwd, wsc, b, y, st, amax, n, L, cin, cout, k, 1, L + 2 * p, 2 * p, det)
    assert bool((y[n * L:] == SENT).all()), "rows past n L written"
    return y, st, amax


def _dgrad(o, dzp, dgr, wsc, case, amax=None):
    cin, L, k, cout, n = case
    p = (k - 1) // 2
    dh = torch.full((n * L + 4, cin), SENT, device=DEV)
    o.gx3_conv(dzp, dgr, wsc, None, dh, None, amax, n, L, cout, cin, k, 2, L + 2 * p, p, False)
    assert bool((dh[n * L:] == SENT).all()), "rows past n L written"
    return dh


def _wgrad(o, xp, dzp, wx, wd, R, cin, cout, k, slices=64):
    wfl = k * cin * cout
    gw = torch.full((wfl + 8,), SENT, device=DEV)
    o.gx3_wgrad(xp, dzp, wx, wd, R, cin, cout, k, gw, torch.empty(slices * wfl, device=DEV))
    assert bool((gw[wfl:] == SENT).all())
    return gw[:wfl].view(k, cin, cout)


def _assert_path(case):
    cin, L, k, cout, n = case
    P = X.conv_path(n, L, cin, cout, k)
    assert (P["path"], P["CT"], P["grid"], P["span"], P["lds"]) == X.CONV_EXPECT[case]
    return P


# ------------------------------------------------------------------------------------------------ exact probes
@pytest.mark.parametrize("case", X.CONV_CASES)
def test_gx3_exact_probes_bitwise(case):
    """Forward (mode 1), dgrad (mode 2) and wgrad on the exact fixtures: ``torch.equal`` to the model tier.
    The kernels of a case together put a weight on every k-row of every tap."""
    o = _ext.ops()
    cin, L, k, cout, n = case
    _assert_path(case)
    dgrad = cin % 4 == 0
    x, dz = X.probe_acts(n, L, cin, 0), X.probe_acts(n, L, cout, 1)
    b = X.probe_bias(cout)
    xin, dzp, bd = _dev(X.padded(x, k, True)), _dev(X.padded(dz, k, False)), _dev(b)
    for i, w in enumerate(X.probe_nets(k, cin, cout, dgrad)):
        M = X.conv_model(x, w, b, relu=True)
        assert X.is_exact(M["y"], M["ab"])
        fwd, dgr, wsc = _pack(o, w, dgrad)
        y, _, _ = _forward(o, xin, fwd, wsc, bd, case, True)
        _bitwise(f"probe forward net {i}", y[: n * L], M["y"])
        if dgrad:
            D = X.conv_model(dz, X.flip_t(w))
            assert X.is_exact(D["y"], D["ab"])
            _bitwise(f"probe dgrad net {i}", _dgrad(o, dzp, dgr, wsc, case)[: n * L], D["y"])
    xp = X.padded(x, k, True)
    R = n * (L + k - 1)
    dzs = X.probe_sparse_dz(R, cout, 0)
    ax, ad = X.amax32(xp), X.amax32(dzs)
    W = X.wgrad_model(xp, dzs, R, k, ax, ad)
    assert X.is_exact(W["gw"], W["ab"])
    _bitwise("probe wgrad", _wgrad(o, xin, _dev(dzs), _word(ax), _word(ad), R, cin, cout, k), W["gw"])


# ------------------------------------------------------------------------------------------------ random cases
def _hold_slots(name, st, u, e, cout):
    """Deterministic table: every slot (workgroup, wave row) against the moments of its own 64 rows."""
    ref = X.slot_moments(u)
    ns = ref.shape[0]
    got = st.view(-1, 2, cout)[:ns].double().cpu()
    worst = 0.0
    for s in range(ns):
        rows = slice(64 * s, min(64 * (s + 1), u.shape[0]))
        a = G.moments_allow(u[rows], e[rows], 8) if rows.start < u.shape[0] else torch.zeros(2, cout, dtype=torch.float64)
        worst = max(worst, X.ratio(got[s] - ref[s], a))
    print(f"[ratio] {name}: {worst:.4f}")
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("case", X.CONV_CASES)
def test_gx3_conv_matches_model_and_float64(case):
    """Mode 1 with atomic slots, then deterministic slots twice (bitwise equal), then mode 2 with the flipped
    fragments; y per entry, moment sums, every deterministic slot, sentinel rows, amax_out."""
    o = _ext.ops()
    cin, L, k, cout, n = case
    P = _assert_path(case)
    R = X.conv_refs(case)
    rows, gx = n * L, P["grid"][0]
    fwd, dgr, wsc = _pack(o, R["w"])
    assert float(wsc.item()) == 2.0 ** -R["fwd"]["sw"]
    xin, bd = _dev(X.padded(R["x"], k, True)), _dev(R["b"])
    u, a1, a2 = R["fwd"]["y"], R["fwd_a1"], R["fwd_a2"]
    true_max = X.amax32(R["x"])
    outs = []
    for det, slots, pre in ((False, 16, 0.0), (True, max(16, 2 * gx), 0.0), (True, max(16, 2 * gx), 4.0 * true_max)):
        y, st, amax = _forward(o, xin, fwd, wsc, bd, case, det, slots, _word(pre))
        assert _as_float(amax) == max(true_max, pre)      # exactly max |x|; a larger word is left alone
        _hold(f"gx3_conv y vs model det={det}", y[:rows], u, a1)
        _hold(f"gx3_conv y vs float64 det={det}", y[:rows], R["fwd_truth"], a1 + a2)
        _hold(f"gx3_conv moments det={det}", st.view(-1, 2, cout).double().sum(0), G.moments64(u),
              G.moments_allow(u, a1, G.conv_chain(rows, det)))
        if det:
            _hold_slots("gx3_conv deterministic slots", st, u, a1, cout)
            assert bool((st.view(-1, 2, cout)[2 * gx:] == 0).all())
        outs.append((y, st))
    _bitwise("gx3_conv deterministic rerun y", outs[1][0], outs[2][0])
    _bitwise("gx3_conv deterministic rerun slots", outs[1][1], outs[2][1])
    if cin % 4 == 0:
        amax = torch.zeros(1, dtype=torch.int32, device=DEV)
        dh = _dgrad(o, _dev(X.padded(R["dz"], k, False)), dgr, wsc, case, amax)
        assert _as_float(amax) == X.amax32(R["dz"])
        _hold("gx3_conv dgrad vs model", dh[:rows], R["dgr"]["y"], R["dgr_a1"])
        _hold("gx3_conv dgrad vs float64", dh[:rows], R["dgr_truth"], R["dgr_a1"] + R["dgr_a2"])
    # one slot too few for the deterministic table: rejected, nothing written
    y = torch.full((rows + 4, cout), SENT, device=DEV)
    st = torch.full(((2 * gx - 1) * 2 * cout,), SENT, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        o.gx3_conv(xin, fwd, wsc, bd, y, st, amax, n, L, cin, cout, k, 1, L + 2 * ((k - 1) // 2), k - 1, True)
    assert bool((y == SENT).all()) and bool((st == SENT).all()) and int(amax.item()) == 0


def test_gx3_conv_rejections():
    """The launcher's own slot check (a table of >= 16 slots that is still one short: 1200 rows need 20) and
    the binding's shape / layout checks; nothing is written."""
    o = _ext.ops()
    cin, L, k, cout, n = 8, 60, 3, 12, 20
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(n, L, cin, generator=g), torch.randn(k, cin, cout, generator=g), torch.zeros(cout)
    fwd, dgr, wsc = _pack(o, w)
    xin, bd = _dev(X.padded(x, k, True)), _dev(b)
    rs = L + 2
    y = torch.full((n * L + 4, cout), SENT, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)

    def st(slots):
        return torch.full((slots * 2 * cout,), SENT, device=DEV)

    assert X.conv_path(n, L, cin, cout, k)["grid"][0] == 10
    bad = [
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(19), amax, n, L, cin, cout, k, 1, rs, 2, True),    # 19 < 20 slots
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(15), amax, n, L, cin, cout, k, 1, rs, 2, False),   # < 16 slots
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax, n, L, cin, cout, k, 3, rs, 2, False),   # mode
        lambda: o.gx3_conv(xin, fwd, wsc, None, y, st(16), amax, n, L, cin, cout, k, 1, rs, 2, False), # no bias
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax, n, L, cin, cout, 4, 1, rs, 2, False),   # even k
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax, n, L, cin, 10, k, 1, rs, 2, False),     # cout % 4
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax, n, L, cin, cout, k, 1, rs, 0, False),   # in_off < pad
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax, n, L, cin, cout, k, 1, L, 1, False),    # in_rs - L < pad
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax, n + 1, L, cin, cout, k, 1, rs, 2, False),  # x, y short
        lambda: o.gx3_conv(xin, dgr, wsc, bd, y, st(16), amax, n, L, cin, cout, k, 1, rs, 2, False),   # wrong fragments
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y[:-5], st(16), amax, n, L, cin, cout, k, 1, rs, 2, False),  # y short
        lambda: o.gx3_conv(xin, fwd, wsc, bd, y, st(16), amax.float(), n, L, cin, cout, k, 1, rs, 2, False),  # amax dtype
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
        assert bool((y == SENT).all()) and int(amax.item()) == 0, i
    y2, _, _ = _forward(o, xin, fwd, wsc, bd, (cin, L, k, cout, n), True, 20)      # exactly enough: accepted
    assert bool((y2[: n * L] != SENT).any())


# ------------------------------------------------------------------------------------------------ mixed magnitudes
def _run_mixed(o, case, x, w, b, dz, packed):
    """Forward (deterministic slots), dgrad where the shape has one, wgrad from the published maxima."""
    cin, L, k, cout, n = case
    fwd, dgr, wsc = packed
    amax = torch.zeros(2, dtype=torch.int32, device=DEV)
    xin, dzp = _dev(X.padded(x, k, True)), _dev(X.padded(dz, k, False))
    y, st, _ = _forward(o, xin, fwd, wsc, _dev(b), case, True, 16, amax[0:1])
    if cin % 4 == 0:
        dh = _dgrad(o, dzp, dgr, wsc, case, amax[1:2])
    else:
        dh = None
        o.gx3_amax(dzp, dzp.numel(), amax[1:2])
    gw = _wgrad(o, xin, dzp, amax[0:1], amax[1:2], dzp.shape[0], cin, cout, k)
    return y[: n * L], st, dh if dh is None else dh[: n * L], gw, amax


@pytest.mark.parametrize("case", X.MIXED_CASES)
def test_gx3_mixed_magnitudes_in_one_workgroup(case):
    """Windows scaled by 2^(0, 12, -18, 5, -7) in one tile: every entry -- the 2^-18 window's included --
    within the allowance with its floor (forward, dgrad, wgrad); x 2^j gives y 2^j, moments 2^j and 2^2j,
    amax 2^j, bit for bit, and dz 2^j the same through dgrad and wgrad."""
    o = _ext.ops()
    cin, L, k, cout, n = case
    x, w, b, dz = X.mixed_fixture(*case)
    assert [t[2:4] for t in X.tiles(x, L)] == [(0, 8), (8, 8)]
    packed = _pack(o, w)
    y, st, dh, gw, amax = _run_mixed(o, case, x, w, b, dz, packed)
    assert _as_float(amax[0:1]) == X.amax32(x) and _as_float(amax[1:2]) == X.amax32(dz)
    F = X.conv_model(x, w, b, relu=True)
    a1 = X.acc_allow(F["ab"], k * cin)
    _hold("mixed forward vs model", y, F["y"], a1)
    _hold("mixed forward vs float64", y, X.conv_truth(x, w, b, True), a1 + X.truth_allow(x, w, F["sb"], F["sw"]))
    _hold_slots("mixed forward slots", st, F["y"], a1, cout)
    if dh is not None:
        wf = X.flip_t(w)
        D = X.conv_model(dz, wf)
        d1 = X.acc_allow(D["ab"], k * cout, extra=1)
        small = slice(5 * L, 6 * L)      # the 2^-18 window of dz
        _hold("mixed dgrad vs model", dh, D["y"], d1)
        _hold("mixed dgrad vs float64", dh, X.conv_truth(dz, wf), d1 + X.truth_allow(dz, wf, D["sb"], D["sw"]))
        _hold("mixed dgrad vs model, 2^-18 window", dh[small], D["y"][small], d1[small])
        # the documented limit: the small window alone against the same window among its tile neighbours
        alone = _dgrad(o, _dev(X.padded(dz[5:6], k, False)), packed[1], packed[2], (cin, L, k, cout, 1))[:L]
        rel = float((dh[small] - alone).abs().max() / alone.abs().max())
        print(f"[figure] neighbour dependence of the 2^-18 window: {rel:.3e} of its largest entry")
        assert rel < 2.0 ** -6
    xp, dzp = X.padded(x, k, True), X.padded(dz, k, False)
    R = dzp.shape[0]
    W = X.wgrad_model(xp, dzp, R, k, X.amax32(x), X.amax32(dz))
    w1 = X.wgrad_acc_allow(W["ab"], R, X.wgrad_path(R, cin, cout, k, 64 * k * cin * cout)[0])
    _hold("mixed wgrad vs model", gw, W["gw"], w1)
    _hold("mixed wgrad vs float64", gw, X.wgrad64(xp, dzp, R, k)[0], w1 + X.wgrad_truth_allow(xp, dzp, R, k, W["sx"], W["sd"]))
    for j in (7, -9):
        s = 2.0 ** j
        y2, st2, dh2, gw2, amax2 = _run_mixed(o, case, x * s, w, b * s, dz * s, packed)
        _bitwise(f"equivariance 2^{j} y", y2, y.cpu().double() * s)
        sl = st.view(-1, 2, cout).cpu().double()
        sl[:, 0] *= s
        sl[:, 1] *= s * s
        _bitwise(f"equivariance 2^{j} moments", st2.view(-1, 2, cout), sl)
        assert _as_float(amax2[0:1]) == X.amax32(x) * s and _as_float(amax2[1:2]) == X.amax32(dz) * s
        if dh is not None:
            _bitwise(f"equivariance 2^{j} dgrad", dh2, dh.cpu().double() * s)
        _bitwise(f"equivariance 2^{j} wgrad (x and dz)", gw2, gw.cpu().double() * s * s)


@pytest.mark.parametrize("case", X.MIXED_CASES)
def test_gx3_window_result_is_independent_of_tile_neighbours(case):
    """Windows within 2^+-5 of each other on a grid coarse enough that their halves are the same at every
    exponent the tile can take (asserted on the CPU): launched from window 3 on, every window reproduces its
    rows of the full launch bit for bit."""
    o = _ext.ops()
    cin, L, k, cout, n = case
    x, w, b = X.neighbour_fixture(*case)
    fwd, dgr, wsc = _pack(o, w)
    bd = _dev(b)
    full, _, _ = _forward(o, _dev(X.padded(x, k, True)), fwd, wsc, bd, case, True)
    sub, _, _ = _forward(o, _dev(X.padded(x[3:], k, True)), fwd, wsc, bd, (cin, L, k, cout, n - 3), True)
    _bitwise("windows 3.. alone", sub[: (n - 3) * L], full[3 * L: n * L])
    _hold("neighbour fixture vs model", full[: n * L], X.conv_model(x, w, b, True)["y"],
          X.acc_allow(X.conv_model(x, w, b, True)["ab"], k * cin))


# ------------------------------------------------------------------------------------------------ gx3_pack
def test_gx3_pack_fragments_bitwise():
    """One launch of eight blocks (``gx3_kernel_refs.PACK_BLOCKS``): forward fragments == split of the Keras
    kernel in fragment order, dgrad fragments == split of the flipped, transposed kernel (block 0 has an empty
    dgrad buffer), zero k tail and channel tail, wsc == 2^-sw, sentinels after every buffer."""
    o = _ext.ops()
    ws = X.pack_weights()
    nb = len(ws)
    GAP = 64
    sizes = [(X.frag_numel(k, ci, co), X.frag_numel(k, co, ci) if i else 0) for i, (k, ci, co) in enumerate(X.PACK_BLOCKS)]
    back = torch.full((sum(a + b + 2 * GAP for a, b in sizes),), SENT, dtype=torch.float16, device=DEV)
    fwd, dgr, spans, off = [], [], [], 0
    for a, b in sizes:
        fwd.append(back[off: off + a])
        dgr.append(back[off + a + GAP: off + a + GAP + b])
        spans += [(off, off + a), (off + a + GAP, off + a + GAP + b)]
        off += a + b + 2 * GAP
    wsc_back = torch.full((nb, 4), SENT, device=DEV)
    wsc = [wsc_back[i, 0:1] for i in range(nb)]
    ks, cis, cos = ([blk[j] for blk in X.PACK_BLOCKS] for j in range(3))
    o.gx3_pack([_dev(w) for w in ws], fwd, dgr, wsc, ks, cis, cos, torch.empty(16 * nb, device=DEV))
    written = torch.zeros(back.numel(), dtype=torch.bool)
    for a, b in spans:
        written[a:b] = True
    assert bool((back.cpu()[~written] == SENT).all()) and bool((wsc_back[:, 1:] == SENT).all())
    for i, w in enumerate(ws):
        ref, sw = X.pack_ref(w, False)
        bad = int((fwd[i].view(torch.int16).cpu() != ref.reshape(-1)).sum())
        print(f"[bitwise] gx3_pack block {i} forward (sw = {sw}): {bad} of {ref.numel()} halves differ")
        assert bad == 0
        assert float(wsc_back[i, 0].item()) == 2.0 ** -sw
        if i:
            ref, _ = X.pack_ref(w, True)
            bad = int((dgr[i].view(torch.int16).cpu() != ref.reshape(-1)).sum())
            print(f"[bitwise] gx3_pack block {i} dgrad: {bad} of {ref.numel()} halves differ")
            assert bad == 0
    with pytest.raises(RuntimeError):      # a fragment buffer of the other orientation's size
        o.gx3_pack([_dev(ws[0])], [dgr[1]], [dgr[0]], [wsc[0]], [7], [3], [20], torch.empty(16, device=DEV))
    with pytest.raises(RuntimeError):      # scratch one float short
        o.gx3_pack([_dev(ws[0])], [fwd[0]], [dgr[0]], [wsc[0]], [7], [3], [20], torch.empty(15, device=DEV))


# ------------------------------------------------------------------------------------------------ gx3_amax
@pytest.mark.parametrize("n", X.AMAX_N)
def test_gx3_amax_edges(n):
    """The maximum in the scalar tail (n % 4 elements after the 16-byte loads), negative; NaN entries are
    skipped, -0.0 counts as 0; nothing past n is read; a larger word already there is left alone."""
    o = _ext.ops()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n + 8, generator=g)
    x[n:] = 1e6
    x[n - 1] = -7.25
    if n >= 3:
        x[0], x[1] = float("nan"), -0.0
    xd = _dev(x)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    o.gx3_amax(xd, n, word)
    assert _as_float(word) == 7.25
    word = _word(9.0)
    o.gx3_amax(xd, n, word)
    assert _as_float(word) == 9.0
    zeros = _dev(torch.full((n + 8,), -0.0))
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    o.gx3_amax(zeros, n, word)
    assert int(word.item()) == 0
    with pytest.raises(RuntimeError):
        o.gx3_amax(xd, n + 9, word)            # more elements than the buffer holds


# ------------------------------------------------------------------------------------------------ gx3_wgrad
@pytest.mark.parametrize("case", X.WGRAD_CASES)
def test_gx3_wgrad_matches_model_and_float64(case):
    """Every row random (the pad rows of x too: the reference is the plain shifted product); two runs bitwise
    equal; amax words 2^10 above the true maxima (the contract is >=) within the allowance whose floor is
    widened by exactly that factor; part one float short is rejected."""
    o = _ext.ops()
    cin, k, cout, n, L, slices = case
    Rf = X.wgrad_refs(case)
    R = Rf["R"]
    assert X.wgrad_path(R, cin, cout, k, slices * k * cin * cout) == X.WGRAD_EXPECT[case]
    xd, dd = _dev(Rf["xp"]), _dev(Rf["dzp"])
    gw = _wgrad(o, xd, dd, _word(Rf["ax"]), _word(Rf["ad"]), R, cin, cout, k, slices)
    _hold("gx3_wgrad vs model", gw, Rf["model"]["gw"], Rf["a1"])
    _hold("gx3_wgrad vs float64", gw, Rf["truth"], Rf["a1"] + Rf["a2"])
    _bitwise("gx3_wgrad rerun", _wgrad(o, xd, dd, _word(Rf["ax"]), _word(Rf["ad"]), R, cin, cout, k, slices), gw)
    up = _wgrad(o, xd, dd, _word(Rf["ax_up"]), _word(Rf["ad_up"]), R, cin, cout, k, slices)
    _hold("gx3_wgrad, amax 2^10 above, vs model", up, Rf["model_up"]["gw"], Rf["a1_up"])
    _hold("gx3_wgrad, amax 2^10 above, vs float64", up, Rf["truth"], Rf["a1_up"] + Rf["a2_up"])
    wfl = k * cin * cout
    out = torch.full((wfl,), SENT, device=DEV)
    for f in (lambda: o.gx3_wgrad(xd, dd, _word(1.0), _word(1.0), R, cin, cout, k, out, torch.empty(wfl - 1, device=DEV)),
              lambda: o.gx3_wgrad(xd[:-1], dd, _word(1.0), _word(1.0), R, cin, cout, k, out, torch.empty(wfl, device=DEV)),
              lambda: o.gx3_wgrad(xd, dd, _word(1.0), _word(1.0), R, cin, cout, k, out[:-1], torch.empty(wfl, device=DEV))):
        with pytest.raises(RuntimeError):
            f()
    assert bool((out == SENT).all())
