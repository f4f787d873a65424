"""Every kernel of the generic layer-wise training path on its own against float64
(``tests/generic_kernel_refs.py``): ``gt_pack``, ``gt_conv`` modes 1 / 2, ``gf_conv``, ``gf_wgrad``,
``gt_wgrad``, ``gt_bn_finalize``, ``gt_apply``, ``gt_bwd`` (both modes), ``gt_bwd_finalize``, ``gt_head``.

The whole-step tests (``test_generic_train_gpu.py``, ``test_fp32_gpu.py``) bound a gradient to a few percent;
a kernel that drops one row, misplaces one tap or routes one pooled gradient to the wrong element of a pair
stays far below that.  Here every entry is held to an allowance derived from the arithmetic alone (fp32
additions at 2^-23, one bf16 store at 2^-8; ``generic_kernel_refs``), on the smallest shapes that reach each
dispatch path; ``test_generic_kernel_refs_cpu.py`` shows that each allowance is at least 10 times smaller than
the effect of such a mistake.  Each test prints its largest |err| / allowance; none may exceed 1."""
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, generic_train

from . import generic_kernel_refs as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 512.0   # sentinel of the rows a kernel must not touch (exact in bf16)


def _ratio(err, allow):
    err, allow = err.abs().reshape(-1), allow.reshape(-1).to(err.dtype)
    inf = torch.full_like(err, float("inf"))
    r = torch.where(allow > 0, err / allow.clamp(min=1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def _hold(name, got, ref, allow, keep=None):
    """Print and assert the largest |got - ref| / allowance (over ``keep`` where given)."""
    err = got.detach().double().cpu().reshape(ref.shape) - ref
    allow = allow.expand(ref.shape) if allow.shape != ref.shape else allow
    if keep is not None:
        err, allow = err[keep], allow[keep]
    r = _ratio(err, allow)
    print(f"[ratio] {name}: {r:.4f}")
    assert r <= 1.0, (name, r)
    return r


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _rows_buffer(v, rs, off, rows, dtype, fill):
    """(n, L, C) placed at rows s rs + off + t of a (rows, C) device buffer prefilled with ``fill``."""
    n, L, C = v.shape
    buf = torch.full((rows, C), fill, dtype=torch.float64)
    G.place_rows(buf, v, rs, off)
    return _dev(buf, dtype)


# ------------------------------------------------------------------------------------------------ gt_pack
def test_gt_pack_fragments_bitwise():
    """One multi-block launch, three different (k, cin, cout): k cin = 21 (not a multiple of 32) with cout 20
    (not a multiple of 16), 100 -> 36, and k = 1 with cout 100.  Forward fragments == ``_frag(w)``, dgrad
    fragments == ``_frag`` of the flipped, transposed kernel, bit for bit."""
    o = _ext.ops()
    blocks = [(7, 3, 20), (5, 20, 36), (1, 36, 100)]
    g = torch.Generator().manual_seed(1)
    ws = [torch.randn(k, ci, co, generator=g) for k, ci, co in blocks]
    fwd = [torch.full(((k * ci + 31) // 32, (co + 15) // 16, 64, 8), SENT, dtype=torch.bfloat16, device=DEV)
           for k, ci, co in blocks]
    dgr = [torch.full(((k * co + 31) // 32, (ci + 15) // 16, 64, 8), SENT, dtype=torch.bfloat16, device=DEV)
           for k, ci, co in blocks]
    o.gt_pack([w.to(DEV) for w in ws], fwd, dgr, [b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks])
    for w, f, d in zip(ws, fwd, dgr):
        assert torch.equal(f.cpu(), generic_train._frag(w))
        assert torch.equal(d.cpu(), generic_train._frag(G.flip_t(w)))


def _pack(o, w, k, cin, cout):
    wd = _dev(w)
    fwd = torch.empty((k * cin + 31) // 32, (cout + 15) // 16, 64, 8, dtype=torch.bfloat16, device=DEV)
    dgr = torch.empty((k * cout + 31) // 32, (cin + 15) // 16, 64, 8, dtype=torch.bfloat16, device=DEV)
    o.gt_pack([wd], [fwd], [dgr], [k], [cin], [cout])
    return fwd, dgr


def _check_moments(name, st, cout, ref, e, chain):
    got = st.view(-1, 2, cout).double().sum(0)
    return _hold(name, got, G.moments64(ref), G.moments_allow(ref, e, chain))


# ------------------------------------------------------------------------------------------------ gt_conv
@pytest.mark.parametrize("cin,L,k,cout,n", G.CONV_CASES)
def test_gt_conv_train_and_dgrad_match_float64(cin, L, k, cout, n):
    """``gt_pack`` + ``gt_conv`` mode 1 (y = relu(conv + b), BN moment slots in atomic and deterministic mode)
    and mode 2 (dgrad by the flipped, transposed kernel) in the padded row layout of ops/generic_train.py
    (in_rs = L + 2 p; in_off = 2 p forward, p dgrad).  The padding rows hold 3.0, not 0: the kernels mask the
    taps outside a sample themselves.  The path each case reaches is named in ``CONV_CASES``."""
    o = _ext.ops()
    x, w, b, dz = G.conv_fixture(cin, L, k, cout, n)
    p, rows, K = (k - 1) // 2, n * L, k * cin
    rs = L + 2 * p
    fwd, dgr = _pack(o, w, k, cin, cout)
    assert torch.equal(fwd.cpu(), generic_train._frag(w))
    wb = w.bfloat16().float()
    xin = _rows_buffer(x, rs, 2 * p, 2 * p + n * rs, torch.bfloat16, 3.0)
    ref, ab = G.conv64(x, wb, b, relu=True), G.conv_abs64(x, wb, b)
    e = G.conv_allow(ref, ab, K, False)
    bd = _dev(b)
    outs = []
    for det, slots in ((False, 16), (True, max(16, 2 * -(-rows // 128))), (True, max(16, 2 * -(-rows // 128)))):
        y = torch.full((rows + 4, cout), SENT, dtype=torch.bfloat16, device=DEV)
        st = torch.zeros(slots * 2 * cout, device=DEV)
        o.gt_conv(xin, fwd, bd, y, st, n, L, cin, cout, k, 1, rs, 2 * p, det)
        assert bool((y[rows:] == SENT).all())
        _hold(f"gt_conv y det={det}", y[:rows], ref.reshape(rows, cout), G.conv_allow(ref, ab, K, True).reshape(rows, cout))
        _check_moments(f"gt_conv moments det={det}", st, cout, ref, e, G.conv_chain(rows, det))
        outs.append((y, st))
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])   # deterministic: bitwise
    if cin % 4 == 0:   # the dgrad's output channels (block 1 of a network has no dgrad)
        dzp = _rows_buffer(dz, rs, p, n * rs, torch.bfloat16, 3.0)
        dh = torch.full((rows + 4, cin), SENT, dtype=torch.bfloat16, device=DEV)
        o.gt_conv(dzp, dgr, None, dh, None, n, L, cout, cin, k, 2, rs, p, False)
        assert bool((dh[rows:] == SENT).all())
        wf = G.flip_t(wb)
        dref, dab = G.conv64(dz, wf), G.conv_abs64(dz, wf)
        _hold("gt_conv dgrad", dh[:rows], dref.reshape(rows, cin), G.conv_allow(dref, dab, k * cout, True).reshape(rows, cin))


# ------------------------------------------------------------------------------------------------ gf_conv / gf_wgrad
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("cin,L,k,cout", G.GF_CASES)
def test_gf_conv_and_wgrad_match_float64(cin, L, k, cout, scale):
    """The exact-fp32 MFMA kernels: products are exact, so no bf16 term; (K + 2) / (R + 2) fp32 additions."""
    o = _ext.ops()
    n = 9
    x, w, b, dz = G.conv_fixture(cin, L, k, cout, n)
    x, b, dz = x * scale, (b * scale).float(), dz * scale
    p, rows, K = (k - 1) // 2, n * L, k * cin
    rs = L + 2 * p
    xin = _rows_buffer(x, rs, 2 * p, 2 * p + n * rs, torch.float32, 3.0 * scale)
    dzp = _rows_buffer(dz, rs, p, n * rs, torch.float32, 3.0 * scale)
    wd, bd = _dev(w), _dev(b)
    ref, ab = G.conv64(x, w, b, relu=True), G.conv_abs64(x, w, b)
    allow = G.conv_allow(ref, ab, K, False)
    outs = []
    for det, slots in ((False, 16), (True, max(16, 2 * -(-rows // 128))), (True, max(16, 2 * -(-rows // 128)))):
        y = torch.full((rows + 4, cout), SENT, device=DEV)
        st = torch.zeros(slots * 2 * cout, device=DEV)
        o.gf_conv(xin, wd, bd, y, st, n, L, cin, cout, k, 1, rs, 2 * p, det)
        assert bool((y[rows:] == SENT).all())
        _hold(f"gf_conv y det={det}", y[:rows], ref.reshape(rows, cout), allow.reshape(rows, cout))
        _check_moments(f"gf_conv moments det={det}", st, cout, ref, allow, G.conv_chain(rows, det))
        outs.append((y, st))
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])
    if cin % 4 == 0:
        dh = torch.full((rows + 4, cin), SENT, device=DEV)
        o.gf_conv(dzp, wd, None, dh, None, n, L, cout, cin, k, 2, rs, p, False)
        assert bool((dh[rows:] == SENT).all())
        wf = G.flip_t(w)
        dref, dab = G.conv64(dz, wf), G.conv_abs64(dz, wf)
        _hold("gf_conv dgrad", dh[:rows], dref.reshape(rows, cin), G.conv_allow(dref, dab, k * cout, False).reshape(rows, cin))
    R = n * rs
    gref, gab = G.wgrad64(xin, dzp, R, k)
    runs = []
    for _ in range(2):
        gw = torch.full((k, cin, cout), SENT, device=DEV)
        part = torch.empty(4 * k * cin * cout, device=DEV)
        o.gf_wgrad(xin, dzp, R, cin, cout, k, gw, part)
        runs.append(gw)
    _hold("gf_wgrad", runs[0], gref, G.wgrad_allow(gab, R, 2))
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ gt_wgrad
@pytest.mark.parametrize("cin,k,cout,n,L", G.WGRAD_CASES)
def test_gt_wgrad_matches_float64(cin, k, cout, n, L):
    """Atomic mode (``part`` None, ``gw`` zeroed) and deterministic mode with a ``part`` of exactly one slice
    (a single row group) and of 16 slices; the path and ``nco`` of each case are named in ``WGRAD_CASES``."""
    o = _ext.ops()
    xp, dzp, R = G.wgrad_fixture(cin, k, cout, n, L)
    xd, dd = _dev(xp, torch.bfloat16), _dev(dzp, torch.bfloat16)
    gref, gab = G.wgrad64(xp, dzp, R, k)
    allow = G.wgrad_allow(gab, R)
    wfl = k * cin * cout
    gw = torch.zeros(k, cin, cout, device=DEV)
    o.gt_wgrad(xd, dd, R, cin, cout, k, gw, None)
    _hold("gt_wgrad atomic", gw, gref, allow)
    for slices in (1, 16):
        runs = []
        for _ in range(2):
            g2 = torch.full((k, cin, cout), SENT, device=DEV)
            o.gt_wgrad(xd, dd, R, cin, cout, k, g2, torch.empty(slices * wfl, device=DEV))
            runs.append(g2)
        _hold(f"gt_wgrad det part={slices}", runs[0], gref, allow)
        assert torch.equal(runs[0], runs[1])
        # deterministic and atomic agree within the allowance
        _hold(f"gt_wgrad det-atomic part={slices}", runs[0], gw.double().cpu(), allow)
    with pytest.raises(RuntimeError):   # one float short of a slice: rejected by the binding, nothing launched
        o.gt_wgrad(xd, dd, R, cin, cout, k, gw, torch.empty(wfl - 1, device=DEV))


# ------------------------------------------------------------------------------------------------ gt_bn_finalize
@pytest.mark.parametrize("C", G.BN_C)
@pytest.mark.parametrize("nslots", G.BN_NSLOTS)
def test_gt_bn_finalize_matches_float64(nslots, C):
    """No conv: a table of partial sums of real fp32 samples.  nslots < 256: one launch; >= 256: the packed
    two-launch slot sum (it consumes the table, hence the clone), with the one-slot tail joining the previous
    range at 257 / 321 / 385.  The near-constant channels (mean 100 / std 0.01, mean 5 / std 1e-3) need the
    normaliser 1 / count as a double: as a float its 2^-24 rounding enters E[u^2] - mean^2 as 2^-24 mean^2."""
    o = _ext.ops()
    worst = 0.0
    for count in G.BN_COUNTS:
        slots, gamma, beta, mmean, mvar = G.bn_fixture(nslots, C, count)
        args = (1.0 / count, gamma, beta, G.EPS, G.MOMENTUM, mmean, mvar)
        ref, allow = G.bn_finalize64(slots, *args), G.bn_finalize_allow(slots, *args)
        st = _dev(slots)
        for update in (True, False):
            mm, mv, bn = _dev(mmean), _dev(mvar), torch.full((4 * C,), SENT, device=DEV)
            o.gt_bn_finalize(st.clone(), C, 1.0 / count, _dev(gamma), _dev(beta), 1e-3, 0.99, mm, mv, update, bn)
            for i, name in enumerate(("scale", "shift", "mean", "rstd")):
                worst = max(worst, _hold(f"bn_finalize {name} count={count}", bn[i * C:(i + 1) * C], ref[i], allow[i]))
            if update:
                worst = max(worst, _hold(f"bn_finalize mmean count={count}", mm, ref[4], allow[4]))
                worst = max(worst, _hold(f"bn_finalize mvar count={count}", mv, ref[5], allow[5]))
            else:
                assert torch.equal(mm.cpu(), mmean) and torch.equal(mv.cpu(), mvar)
    print(f"[ratio] bn_finalize nslots={nslots} C={C} worst: {worst:.4f}")


# ------------------------------------------------------------------------------------------------ elementwise
def _skey_i32(k):
    return k - (1 << 32) if k >= (1 << 31) else k


def _elem_cases():
    base = [(bf16, C, n, L) for bf16 in (True, False) for C in G.ELEM_C for (n, L) in G.ELEM_NL]
    return base + G.ELEM_EXTRA


@pytest.mark.parametrize("bf16,C,n,L", _elem_cases())
def test_gt_apply_and_bwd_match_float64(bf16, C, n, L):
    """``gt_apply``, ``gt_bwd`` (stats and dz mode, tensor and head upstream), ``gt_bwd_finalize`` on one
    fixture per variant (pool, dropout rate, window offset: ``elem_variants``).  C = 4: G = 1 channel group,
    256 row lanes; C = 1024: G = 256, one row lane.  A 16-slot deterministic table caps the grid (grid-stride
    rows) wherever the launch would have more than 16 blocks: every C >= 256 case with n L >= 45, and the
    G = 1 case of 18000 rows (``ELEM_EXTRA``)."""
    o = _ext.ops()
    dt = _dt(bf16)
    rows = n * L
    for vi, (pool, rate, woff) in enumerate(G.elem_variants(bf16, C, n, L)):
        head = bool(vi & 1)
        F = G.elem_fixture(bf16, C, n, L, pool, rate, woff, head=head)
        tag = f"pool={int(pool)} rate={rate} woff={woff} head={int(head)}"
        lout, drop, ik, thr = F["lout"], rate > 0, F["ik"], F["thr"]
        z = _dev(F["z"].reshape(rows, C), dt)
        bn = _dev(F["bn"].reshape(-1))
        kd = torch.tensor([_skey_i32(G.SKEY)], dtype=torch.int32, device=DEV)
        wrong = G.SKEY ^ 0x5A5A5A5A
        # ---- gt_apply: rows outside s out_rs + out_off + [0, lout) keep the sentinel
        out_rs, out_off = lout + 3, 2
        nrows = n * out_rs + 4
        idx = G.row_index(n, lout, out_rs, out_off)
        outs = []
        for skey, dev_key in ((G.SKEY, None), (wrong, kd)):   # by value; through skey_dev (which must win)
            out = torch.full((nrows, C), SENT, dtype=dt, device=DEV)
            o.gt_apply(z, bn, out, n, L, C, pool, out_rs, out_off, drop, thr, ik, skey, woff, dev_key)
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        out = outs[0].double().cpu()
        other = torch.ones(nrows, dtype=torch.bool)
        other[idx] = False
        assert bool((out[other] == SENT).all())
        if lout > 0:
            got, ref = out[idx], F["y"].reshape(n * lout, C)
            if drop:
                keep = F["keep"].reshape(n * lout, C)
                assert bool((got[~keep] == 0).all())                      # the mask is exact
                assert bool((got[keep & (ref != 0)] != 0).all())
            _hold(f"gt_apply {tag}", got, ref, G.apply_allow(ref, F["ymag"].reshape(n * lout, C), bf16))
        # ---- upstream gradient
        if head:
            up = dict(dh=None, dlog=_dev(F["dlog"]), w=_dev(F["w"]), invL=F["invL"])
        else:
            up = dict(dh=_dev(F["dh"].reshape(n * lout, C), dt) if lout > 0 else torch.zeros(1, C, dtype=dt, device=DEV),
                      dlog=None, w=None, invL=1.0)
        ex = G.excluded_rows(F)
        okc = ~ex.reshape(rows, C).any(0)   # channels without an excluded pool pair
        # ---- gt_bwd stats mode: atomic (16 slots), deterministic (256 slots; 16 slots: the capped grid)
        for det, slots in ((False, 16), (True, 256), (True, 16)):
            tabs = []
            for rep in range(2 if det else 1):
                bst = torch.zeros(slots * 2 * C, device=DEV)
                skey, dev_key = ((G.SKEY, None), (wrong, kd))[rep]
                o.gt_bwd(False, z, bn, up["dh"], up["dlog"], up["w"], up["invL"], n, L, C, pool, drop, thr, ik, skey, woff,
                         bst, None, None, None, 0, 0, None, dev_key, det)
                tabs.append(bst)
            if det:
                assert torch.equal(tabs[0], tabs[1])   # bitwise run to run, and the device key wins
            got = tabs[0].view(slots, 2, C).double().sum(0)
            chain = G.bwd_chain(rows, C, slots, det)
            _hold(f"gt_bwd stats det={det} slots={slots} {tag}", got, F["sums"], chain * G.U32 * F["sums_abs"],
                  keep=okc[None, :].expand(2, C))
            # ---- gt_bwd_finalize: both jobs; the bias side job on a table of another width (BC != C)
            BC = C + 4
            gsl = torch.Generator().manual_seed(slots + C)
            dbs = torch.randn(slots, BC, generator=gsl)
            coef, gg, gbt = (torch.full((2 * C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV),
                             torch.full((C,), SENT, device=DEV))
            gbias = torch.full((BC,), SENT, device=DEV)
            o.gt_bwd_finalize(tabs[0], C, F["inv_count"], coef, gg, gbt, _dev(dbs), gbias)
            s64 = tabs[0].view(slots, 2, C).double().cpu()
            tot, tab_abs = s64.sum(0), s64.abs().sum(0)
            _hold(f"gt_bwd_finalize gbeta {tag}", gbt, tot[0], 2.0 ** -23 * tab_abs[0])
            _hold(f"gt_bwd_finalize ggamma {tag}", gg, tot[1], 2.0 ** -23 * tab_abs[1])
            _hold(f"gt_bwd_finalize coef {tag}", coef.view(2, C), tot * F["inv_count"], 2.0 ** -23 * tab_abs * F["inv_count"])
            _hold(f"gt_bwd_finalize bias BC={BC} {tag}", gbias, dbs.double().sum(0), 2.0 ** -23 * dbs.double().abs().sum(0))
        # ---- gt_bwd dz mode: padded layout with sentinels, exact zeros under the ReLU, bias slots
        dz_rs, dz_off = L + 3, 1
        drows = n * dz_rs + 4
        didx = G.row_index(n, L, dz_rs, dz_off)
        cf, gm = _dev(F["coef"].reshape(-1)), _dev(F["gamma"])
        dref, dmag = F["dz"].reshape(rows, C), F["dzmag"].reshape(rows, C)
        for det, slots in ((False, 16), (True, 256), (True, 16)):
            runs = []
            for rep in range(2 if det else 1):
                dzb = torch.full((drows, C), SENT, dtype=dt, device=DEV)
                gsl = torch.zeros(slots, C, device=DEV)
                skey, dev_key = ((G.SKEY, None), (wrong, kd))[rep]
                o.gt_bwd(True, z, bn, up["dh"], up["dlog"], up["w"], up["invL"], n, L, C, pool, drop, thr, ik, skey, woff,
                         None, cf, gm, dzb, dz_rs, dz_off, gsl, dev_key, det)
                runs.append((dzb, gsl))
            if det:
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            dzb = runs[0][0].double().cpu()
            other = torch.ones(drows, dtype=torch.bool)
            other[didx] = False
            assert bool((dzb[other] == SENT).all())
            got = dzb[didx]
            assert bool((got[F["z"].reshape(rows, C) <= 0] == 0).all())
            _hold(f"gt_bwd dz det={det} slots={slots} {tag}", got, dref, G.dz_allow(dref, dmag, bf16), keep=~ex.reshape(rows, C))
            # the bias gradient: gt_bwd_finalize with C = 0 sums the slots (the fp32 dz before its store)
            gbias = torch.full((C,), SENT, device=DEV)
            none = torch.zeros(4, device=DEV)
            o.gt_bwd_finalize(none, 0, 1.0, none, none, none, runs[0][1], gbias)
            chain = G.bwd_chain(rows, C, slots, det)
            a = chain * G.U32 * dref.abs().sum(0) + (2.0 ** -20 * dmag).sum(0)
            _hold(f"gt_bwd bias det={det} slots={slots} {tag}", gbias, dref.sum(0), a, keep=okc)


@pytest.mark.parametrize("C", [1028, 6])
def test_elementwise_bindings_reject_bad_channel_counts(C):
    """C > 1024 (more channel groups than threads) and C not a multiple of 4: refused before any launch."""
    o = _ext.ops()
    z = torch.zeros(8, C, device=DEV)
    bn = torch.zeros(4 * C, device=DEV)
    with pytest.raises(RuntimeError):
        o.gt_apply(z, bn, torch.zeros(8, C, device=DEV), 2, 4, C, False, 4, 0, False, 0, 1.0, 0, 0, None)
    with pytest.raises(RuntimeError):
        o.gt_bwd(False, z, bn, z, None, None, 1.0, 2, 4, C, False, False, 0, 1.0, 0, 0, torch.zeros(32 * C, device=DEV),
                 None, None, None, 0, 0, None, None, False)


# ------------------------------------------------------------------------------------------------ gt_head
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("C,L,n", G.HEAD_CASES)
def test_gt_head_matches_float64(C, L, n, bf16):
    """n < 4 (one partly filled workgroup), a ragged last workgroup (n = 5, 130), many workgroups (130);
    dense biases 0.25 and +-30 (saturated sigmoid, log1pf(exp(-|z|))).  Atomic mode with zeroed accumulators;
    deterministic mode with a ``part`` of exactly ceil(n / 4) (C + 2) floats, bitwise run to run."""
    o = _ext.ops()
    h, w, y = G.head_fixture(C, L, n, bf16)
    hd, wd, yd = _dev(h.reshape(n * L, C), _dt(bf16)), _dev(w), _dev(y)
    inv_gb = 1.0 / n
    nrec = -(-n // 4) * (C + 2)
    for bias in G.HEAD_BIASES:
        b = torch.tensor([bias], dtype=torch.float64)
        ref = G.head64(h, w, b, y, inv_gb)
        allow = G.head_allow(ref, n, C, inv_gb)
        bd = _dev(b)
        runs = []
        for part in (None, nrec, nrec):
            prob, dlog = torch.full((n,), SENT, device=DEV), torch.full((n,), SENT, device=DEV)
            fill = 0.0 if part is None else SENT   # deterministic mode overwrites its outputs
            loss, gb, gw = (torch.full((1,), fill, device=DEV), torch.full((1,), fill, device=DEV),
                            torch.full((C,), fill, device=DEV))
            o.gt_head(hd, wd, bd, yd, prob, dlog, loss, gw, gb, n, L, C, inv_gb,
                      None if part is None else torch.empty(part, device=DEV))
            mode = "atomic" if part is None else "det"
            if len(runs) < 2:
                # the dense gradients against sum dlog g of the kernel's own dlog (held to float64 just before)
                rk = G.head64(h, w, b, y, inv_gb, dlog=dlog)
                ak = G.head_allow(rk, n, C, inv_gb)
                for name, got, r, a in (("prob", prob, ref, allow), ("dlog", dlog, ref, allow), ("loss", loss, ref, allow),
                                        ("gw", gw, rk, ak), ("gb", gb, rk, ak)):
                    _hold(f"gt_head {name} {mode} bias={bias}", got, r[name].reshape(got.shape), a[name].reshape(got.shape))
            runs.append((prob, dlog, loss, gw, gb))
        assert all(torch.equal(a, c) for a, c in zip(runs[1], runs[2]))
    if nrec > 1:
        with pytest.raises(RuntimeError):   # one float short: rejected by the binding, nothing launched
            o.gt_head(hd, wd, bd, yd, prob, dlog, loss, gw, gb, n, L, C, inv_gb, torch.empty(nrec - 1, device=DEV))
