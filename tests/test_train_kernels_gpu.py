"""Every kernel of the dedicated training path (``csrc/train_fwd.hip``, ``train_head.hip``, ``train_dgrad.hip``, ``train_wgrad.hip``, ``train_reduce.hip``) launched
ALONE through ``torch.ops.apneauq.train_call`` on a ``TrainWorkspace`` whose input buffers the test fills
itself, and held per entry to the float64 references and allowances of ``tests/train_kernel_refs.py``.

The whole-step test (``test_train_gpu.py``) bounds a gradient to 12 %; a wrong halo row at one tile edge, a
prefetched tile staged one row off, a row group counted twice or a mask drawn with the wrong layer id stay
far below that.  Here no kernel's error leaks into the next one's test, the shapes are the smallest at which
each dispatch path is taken (derived from the launch code's thresholds, read through ``train_kernel_refs.geo``), and
``test_train_kernel_refs_cpu.py`` shows that each allowance is at least 10 times smaller than the effect of
such a mistake.  Each check prints its largest |err| / allowance; none may exceed 1."""
import functools

import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models.cnn import AlarconCNN1D
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, train_ops

from . import train_kernel_refs as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7            # the models' dropout seed
SENT = 512.0        # sentinel of rows a kernel must not touch (exact in bf16)
STALE = 3.0         # stale data of a larger, earlier batch in the rows beyond this one's tiles
NEG0 = -32768       # the bit pattern of a bf16 -0.0 as int16


def _ratio(err, allow):
    err, allow = err.abs().reshape(-1), allow.reshape(-1)
    inf = torch.full_like(err, float("inf"))
    r = torch.where(allow > 0, err / allow.clamp(min=1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def _hold(name, got, ref, allow):
    """Print and assert the largest |got - ref| / allowance."""
    ref = ref.to(DEV)
    allow = torch.as_tensor(allow, dtype=torch.float64, device=DEV)
    if allow.shape != ref.shape:
        allow = allow.expand(ref.shape)
    r = _ratio(got.detach().double().reshape(ref.shape) - ref, allow.contiguous())
    print(f"[ratio] {name}: {r:.4f}")
    assert r <= 1.0, (name, r)
    return r


@functools.lru_cache(maxsize=None)
def _model(pseed):
    m = AlarconCNN1D(seed=SEED, device=torch.device(DEV))
    for k, v in T.params(pseed).items():
        m.store.views[k].copy_(v)
    return m


_workspaces = {}


def _ws(n_alloc, det=False, pseed=3):
    """One workspace per (capacity, mode, parameter set), shared by the tests; every test fills what it reads."""
    key = (n_alloc, det, pseed)
    if key not in _workspaces:
        if len(_workspaces) >= 4:        # the large ones hold a few hundred MB each
            _workspaces.clear()
            torch.cuda.empty_cache()
        ws = train_ops.TrainWorkspace(_model(pseed), n_alloc, deterministic=det)
        ws.pack()
        _workspaces[key] = ws
    ws = _workspaces[key]
    ws.full = (ws.wpart, ws.hpart)
    return ws


@pytest.fixture(scope="module", autouse=True)
def _release_workspaces():
    """The shared workspaces and models go when the file is done (the large ones hold over a GB)."""
    yield
    _workspaces.clear()
    _model.cache_clear()
    torch.cuda.empty_cache()


def _ctx(ws, n, dropout=True, table=True, wpart=True, hpart=True, counters=False, seed=SEED):
    ws.wpart, ws.hpart = (ws.full[0] if wpart else None), (ws.full[1] if hpart else None)
    ws._ctx_key = None
    ctx = ws.build_ctx(n, n, 1, 0, seed, dropout, 1.0 / (n * T.L), 1.0 / n, device_counters=counters,
                       table=table and wpart)
    ws.wpart, ws.hpart = ws.full
    ws._ctx_key = None
    return ctx


def _call(ctx, op, layer=0, flag=0):
    train_ops._call(ctx, op, layer, flag, T.PASS, 0)


def _p(ws, name):
    return ws.model.store.views[name]


def _dev(t, dtype=torch.float64):
    return t.to(DEV).to(dtype)


# ---- filling the padded-row buffers
def _fill_rows(buf, v, n, outside=SENT):
    """``buf`` (rows, C) := ``v`` (n, 60, C) on the valid rows; -0.0 on the halo / pad rows of the n samples'
    tiles and on the rows of an odd batch's missing sample (what the producing kernel leaves there);
    ``outside`` on every row beyond the last tile."""
    end = T.HALO + 128 * T.tiles(n)
    buf.fill_(outside)
    buf[:end].fill_(-0.0)
    T.place(buf, v)
    return buf


def _put_R(ws, l, mag, drop, n):
    return _fill_rows(ws.R[l], T.encode(mag, drop).to(DEV), n, outside=STALE)


def _put_grad(buf, v, n):
    """A gradient buffer (dY / dZ): zeros where the producing dgrad writes zeros."""
    end = T.HALO + 128 * T.tiles(n)
    buf.fill_(STALE)
    buf[:end].zero_()
    T.place(buf, v.to(DEV))
    return buf


def _put_slots(dst, slots):
    dst.copy_(slots.to(DEV).reshape(-1))


def _put_tab(ws, l, **rows):
    tab = ws.tab.view(6, T.TAB_ROWS, 256)
    idx = dict(mean=T.T_MEAN, rstd=T.T_RSTD, s=T.T_S, t=T.T_T, mdy=T.T_MDY, mdyx=T.T_MDYX)
    for k, v in rows.items():
        tab[l, idx[k], : v.numel()] = v.to(DEV).float()


def _tab_rows(ws, l):
    """The fp32 table rows of block l, as float64 on the device."""
    tab = ws.tab.view(6, T.TAB_ROWS, 256)[l, :, : T.CH[l + 1]].double()
    return dict(mean=tab[T.T_MEAN], rstd=tab[T.T_RSTD], s=tab[T.T_S], t=tab[T.T_T], mdy=tab[T.T_MDY], mdyx=tab[T.T_MDYX])


def _check_rows_outside(name, buf, n, before, zero_bits):
    """Pad / out-of-batch rows inside the tile range hold ``zero_bits`` (-0.0 for R, +0.0 for gradients), the
    rows beyond the last tile what they held ``before``."""
    rows = buf.shape[0]
    end = T.HALO + 128 * T.tiles(n)
    inside = torch.zeros(rows, dtype=torch.bool)
    inside[:end] = True
    pad = (inside & ~T.valid_rows(rows, n)).to(DEV)
    bits = buf.view(torch.int16)
    assert bool((bits[pad] == zero_bits).all()), name + ": pad / out-of-batch rows"
    assert bool((buf[end:] == before).all()), name + ": rows beyond the last tile touched"


# ================================================================================================ table / finalize
N_BN = T.BN_COUNT // T.L     # 64 samples: a count of 3840


def _edge_slots(ws):
    """Every block's moment slots := the edge channels of ``bn_edge_slots``, gamma[2] := 1 on every block."""
    sl = []
    for l in range(6):
        s = T.bn_edge_slots(T.CH[l + 1], l)
        _put_slots(ws.st[l], s)
        _p(ws, f"batchnorm_{l + 1}/gamma")[2] = 1.0
        sl.append(s.to(DEV))
    return sl


def _restore_gamma(ws):
    for l in range(6):
        _p(ws, f"batchnorm_{l + 1}/gamma")[2] = 0.0


def _check_fwd_rows(ws, sl, tag):
    worst = {}
    for l in range(6):
        gamma, beta = _p(ws, f"batchnorm_{l + 1}/gamma"), _p(ws, f"batchnorm_{l + 1}/beta")
        r = T.bn_rows64(sl[l], 1.0 / T.BN_COUNT, gamma, beta)
        al = T.bn_rows_allow(r, gamma, beta)
        got = _tab_rows(ws, l)
        for k in ("mean", "rstd", "s", "t"):
            # the near-constant channel (2) on its own line: the row a float normaliser breaks
            _hold(f"table {tag} block {l} {k} near-constant channel", got[k][2], r[k][2], al[k][2])
            worst[k] = max(worst.get(k, 0.0), _hold(f"table {tag} block {l} {k}", got[k], r[k], al[k]))
    return worst


@pytest.mark.parametrize("how", ["op5", "head"])
def test_table_forward_rows_match_float64(how):
    """Forward rows (mean, rstd, s, t) of all six blocks from moment slots the test wrote: a near-constant
    channel far from zero at a count of 3840 (mean 100, std 0.01), a channel of variance exactly 0, one of huge
    variance.  By ``tab_kernel`` (op 5) and by the head launch's extra workgroups (op 1, flag bit 1)."""
    ws = _ws(N_BN)
    sl = _edge_slots(ws)
    try:
        ws.tab.fill_(SENT)
        ctx = _ctx(ws, N_BN)
        if how == "op5":
            _call(ctx, 5, 0, 0)
        else:
            ws.R[5].fill_(-0.0)
            _call(ctx, 1, 0, 2)
        _check_fwd_rows(ws, sl, how)
        tab = ws.tab.view(6, T.TAB_ROWS, 256)
        assert bool((tab[:, T.T_MDY:] == SENT).all())          # the backward rows are not this launch's
        for l in range(6):
            assert bool((tab[l, :, T.CH[l + 1]:] == SENT).all())
    finally:
        _restore_gamma(ws)


def test_table_backward_rows_match_float64():
    """op 5 flag 1: mean dY, mean dY xhat of one block from its fp64 backward slots."""
    ws = _ws(N_BN)
    ctx = _ctx(ws, N_BN)
    for l in range(6):
        C = T.CH[l + 1]
        bst = torch.randn(T.SLOTS, 2, C, generator=T._gen(21, l), dtype=torch.float64) * 1e-3
        _put_slots(ws.bst[l], bst)
        ws.tab.fill_(SENT)
        _call(ctx, 5, l, 1)
        ref, al = T.slot_mean64(bst.to(DEV), 1.0 / T.BN_COUNT)
        got = _tab_rows(ws, l)
        _hold(f"table backward rows block {l}", torch.stack([got["mdy"], got["mdyx"]]), ref, al)
        assert bool((ws.tab.view(6, T.TAB_ROWS, 256)[l, : T.T_MDY] == SENT).all())


@pytest.mark.parametrize("update_moving,grads", [(1, 1), (1, 0), (0, 1)])
def test_finalize_matches_float64(update_moving, grads):
    """``bn_finalize_kernel`` (op 4): the moving mean / variance update from the edge-channel slots, dgamma /
    dbeta from the backward slots, and the head's slotted sums (dense-weight gradient, loss, dense-bias
    gradient) added in slot order."""
    ws = _ws(N_BN)
    sl = _edge_slots(ws)
    _restore_gamma(ws)
    ctx = _ctx(ws, N_BN)
    C6 = T.CH[6]
    hp = torch.randn(T.SLOTS, C6 + 2, generator=T._gen(22)).to(DEV)
    ws.hpart.copy_(hp.reshape(-1))
    before, bsts = {}, []
    for l in range(6):
        i = l + 1
        g = T._gen(23, l)
        _p(ws, f"batchnorm_{i}/moving_mean").copy_(torch.randn(T.CH[i], generator=g))
        _p(ws, f"batchnorm_{i}/moving_variance").copy_(0.5 + torch.rand(T.CH[i], generator=g))
        before[l] = (_p(ws, f"batchnorm_{i}/moving_mean").clone(), _p(ws, f"batchnorm_{i}/moving_variance").clone())
        bsts.append(torch.randn(T.SLOTS, 2, T.CH[i], generator=g, dtype=torch.float64).to(DEV))
        _put_slots(ws.bst[l], bsts[l])
    ws.grad.fill_(SENT)
    ws.loss.fill_(SENT)
    _call(ctx, 4, update_moving, grads)
    for l in range(6):
        i = l + 1
        ref, al = T.finalize64(sl[l], bsts[l], 1.0 / T.BN_COUNT, before[l][0], before[l][1], hp if l == 5 else None)
        mm, mv = _p(ws, f"batchnorm_{i}/moving_mean"), _p(ws, f"batchnorm_{i}/moving_variance")
        if update_moving:
            _hold(f"finalize block {l} moving mean", mm, ref["mmean"], al["mmean"])
            _hold(f"finalize block {l} moving variance", mv, ref["mvar"], al["mvar"])
        else:
            assert torch.equal(mm, before[l][0]) and torch.equal(mv, before[l][1])
        gg, gb = ws.gviews[f"batchnorm_{i}/gamma"], ws.gviews[f"batchnorm_{i}/beta"]
        if grads:
            _hold(f"finalize block {l} dgamma", gg, ref["ggamma"], al["ggamma"])
            _hold(f"finalize block {l} dbeta", gb, ref["gbeta"], al["gbeta"])
        else:
            assert bool((gg == SENT).all()) and bool((gb == SENT).all())
    head = torch.cat([ws.gviews["output_layer/kernel"].reshape(-1), ws.loss.reshape(-1),
                      ws.gviews["output_layer/bias"].reshape(-1)])
    if grads:
        _hold("finalize head sums", head, ref["head"], al["head"])
    else:
        assert bool((head == SENT).all())


# ================================================================================================ head
def _head_case(ws, n, bias, dropout, seed=SEED, tag=0):
    """R_6 with sample 0 dropped whole (n >= 2), labels, the dense bias; -> the float64 inputs on the device."""
    mag, drop = T.act_fixture(5, n, seed, dropout, tag)
    if n >= 2 and dropout:
        drop[0] = True
    _put_R(ws, 5, mag, drop, n)
    y = (torch.rand(n, generator=T._gen(24, n, tag)) > 0.5).float()
    ws.y.fill_(STALE)
    ws.y[:n] = y.to(DEV)
    assert abs(bias) != 30.0 or 0 < int(y.sum()) < n          # a saturated logit meets both labels
    _p(ws, "output_layer/bias").fill_(bias)
    return _dev(mag), drop.to(DEV), _dev(y)


HEAD_N = [2051, 4099]     # 2051: 2 samples per wave; 4099: 4 (over 512 workgroups each)
HEAD_CASES = [(n, n, "table", 0.25, True) for n in (1, 2, 37)] + [(3, 8, "table", 0.25, True)] + \
             [(n, n, "table", 0.25, True) for n in HEAD_N] + \
             [(37, 37, m, 0.25, True) for m in ("slots", "atomic", "det")] + \
             [(37, 37, "table", b, True) for b in (30.0, -30.0)] + [(37, 37, "atomic", 30.0, True)] + \
             [(37, 37, "table", 0.25, False)]


@pytest.mark.parametrize("n,n_alloc,mode,bias,dropout", HEAD_CASES)
def test_head_matches_float64(n, n_alloc, mode, bias, dropout):
    """``head_kernel`` (op 1, backward): logits, dlogit, and the sums -- loss, dense-weight and dense-bias
    gradients (through the slots of ``hpart``, by direct atomics, or from the deterministic records), the
    backward sums of block 6.  'table': BN rows from a table the test wrote; 'slots' / 'atomic' / 'det': from
    the moment slots (rows taken from what op 5 writes for the same slots).  One sample has all 96 channels
    dropped, gamma is 0 on channel 2, a dense bias of +-30 saturates every logit with both labels present."""
    spw = [T.geo(v)["head"]["spw"] for v in HEAD_N]
    assert spw == [2, 4] and all(v % (4 * k) for v, k in zip(HEAD_N, spw))
    ws = _ws(n_alloc, mode == "det")
    S = _head_prepare(ws, n, mode, bias, dropout)
    _call(S["ctx"], 1, 0, 1)
    _head_check(ws, S)


def _head_prepare(ws, n, mode, bias, dropout, seed=SEED, tag=0, counters=False):
    det = mode == "det"
    n_alloc = ws.B
    ws.zero_accumulators()
    mag, drop, y = _head_case(ws, n, bias, dropout, seed, tag)
    gamma, beta = _p(ws, "batchnorm_6/gamma"), _p(ws, "batchnorm_6/beta")
    rows = {k: v.to(DEV) for k, v in T.table_rows(mag.cpu(), gamma.cpu(), beta.cpu(), n).items()}
    if mode == "table":
        ws.tab.fill_(SENT)
        _put_tab(ws, 5, **rows)
        ctx = _ctx(ws, n, dropout, counters=counters, seed=seed)
    else:
        _put_slots(ws.st[5], T.moment_slots(mag))
        if det:      # no table in deterministic mode: the rows come from an atomic-mode twin's op 5
            tw = _ws(n_alloc, False)
            _put_slots(tw.st[5], T.moment_slots(mag))
            _call(_ctx(tw, n, dropout), 5, 0, 0)
            rows = _tab_rows(tw, 5)
        else:
            _call(_ctx(ws, n, dropout), 5, 0, 0)
            rows = _tab_rows(ws, 5)
        ctx = _ctx(ws, n, dropout, table=False, hpart=(mode == "slots"))
    for t in (ws.logits, ws.dlogit):
        t.fill_(SENT)
    return dict(ctx=ctx, mag=mag, drop=drop, y=y, rows=rows, n=n, mode=mode, bias=bias, dropout=dropout, tag=tag)


def _head_check(ws, S, M=1):
    mag, drop, y, rows, n, mode, bias, dropout = (S[k] for k in ("mag", "drop", "y", "rows", "n", "mode", "bias", "dropout"))
    ib = 1.0 / n
    sc = T.dsc(5) if dropout else 1.0
    w = _p(ws, "output_layer/kernel").double()
    r = T.head64(mag, drop, rows, w, bias, y, ib, sc, dlog=ws.dlogit[:n])
    al = T.head_allow(r, n, ib, "slots" if mode == "table" else mode, M)
    tag = f"head n={n} {mode} b={bias:g}" + ("" if dropout else " no-dropout") + (f" member {S['tag']} of {M}" if M > 1 else "")
    _hold(tag + " logits", ws.logits[:n], r["logit"], al["logit"])
    _hold(tag + " dlogit", ws.dlogit[:n], r["dlog"], al["dlog"])
    assert bool((ws.logits[n:] == SENT).all()) and bool((ws.dlogit[n:] == SENT).all())
    if n >= 2 and dropout:
        assert float(ws.logits[0]) == float(torch.tensor(bias).float())       # every channel dropped
    if abs(bias) == 30.0:
        assert bool((ws.dlogit[:n] != 0).all())                              # saturated, never cancelled to 0
    C6 = T.CH[6]
    if mode in ("table", "slots"):
        h = ws.hpart.view(T.SLOTS, C6 + 2).double().sum(0)
        gw, loss, gb = h[:C6], h[C6], h[C6 + 1]
    else:
        gw, loss, gb = ws.gviews["output_layer/kernel"].reshape(-1), ws.loss[0], ws.gviews["output_layer/bias"][0]
    _hold(tag + " loss", loss, r["loss"], al["loss"])
    _hold(tag + " dense-weight gradient", gw, r["gw"], al["gw"])
    _hold(tag + " dense-bias gradient", gb, r["gb"], al["gb"])
    _hold(tag + " bst[5]", ws.bst[5].view(T.SLOTS, 2, C6).sum(0), r["bst"], al["bst"])
    _p(ws, "output_layer/bias").fill_(0.25)


# ================================================================================================ forward
def _fwd_inputs(ws, l, n, dropout, seed=SEED, tag=0):
    """Fill block l's input (x, or R_{l-1} and block l-1's moment slots) -> (A, amb) the kernel stages."""
    if l == 0:
        x = T.bf(torch.randn(n, T.L, T.CH[0], generator=T._gen(25, n, tag)).double())
        ws.x.fill_(STALE)
        ws.x[: T.HALO + 128 * T.tiles(n)].zero_()
        T.place(ws.x, x.to(DEV))
        return _dev(x), None
    mag, drop = T.act_fixture(l - 1, n, seed, dropout, tag)
    _put_R(ws, l - 1, mag, drop, n)
    mag, drop = _dev(mag), drop.to(DEV)
    _put_slots(ws.st[l - 1], T.moment_slots(mag))
    # the staging's fp32 s, t: what op 5 writes for the same slots (tab_write_fwd / bn_affine_to_lds)
    tw = ws if ws.det is None else _ws(ws.B, False)
    if tw is not ws:
        _put_slots(tw.st[l - 1], T.moment_slots(mag))
    _call(_ctx(tw, n, dropout, seed=seed), 5, 0, 0)
    rows = _tab_rows(tw, l - 1)
    return T.stage64(mag, drop, rows["s"], rows["t"], T.dsc(l - 1) if dropout else 1.0)


FWD_BIG = [1026, 1024]     # 1026: 513 tiles (prefetching persistent); 1024: plain
FWD_CASES = [(l, n, n, "atomic", True) for l in range(6) for n in (1, 2, 37)] + \
            [(l, 3, 8, "atomic", True) for l in range(6)] + \
            [(l, n, n, "atomic", True) for l in (1, 3) for n in FWD_BIG] + \
            [(l, 37, 37, "det", True) for l in (0, 2, 5)] + [(l, 37, 37, "atomic", False) for l in (0, 4)]


@pytest.mark.parametrize("l,n,n_alloc,mode,dropout", FWD_CASES)
def test_fwd_matches_float64(l, n, n_alloc, mode, dropout):
    """``fwd_kernel<l>`` (op 0): |stored R_l| against relu(conv(A_{l-1}) + b) with the staging's inner bf16
    rounding reproduced (ambiguous inputs widen exactly the entries reading them), the mask sign bits exact
    against ``rng.keep_mask_torch``, -0.0 on every pad and out-of-batch row, the rows beyond the last tile
    untouched, and the moment slots against the moments of the stored tile.  Channel 0 has zero weights and
    bias (kept zeros are +0.0, dropped ones -0.0), channel 1 a bias of -50."""
    assert [T.tiles(v) - T.geo(v)["fwd_train_grid"] for v in FWD_BIG] == [1, 0]      # either side of the threshold
    assert [[T.geo(v)["blocks"][b]["fwd"]["pf"] for b in (1, 3)] for v in FWD_BIG] == [[True, True], [False, False]]
    ws = _ws(n_alloc, mode == "det")
    S = _fwd_prepare(ws, l, n, mode, dropout)
    _call(S["ctx"], 0, l, 0)
    _fwd_check(ws, S)


def _fwd_prepare(ws, l, n, mode, dropout, seed=SEED, tag=0, counters=False):
    a, amb = _fwd_inputs(ws, l, n, dropout, seed, tag)
    end = T.HALO + 128 * T.tiles(n)
    R = ws.R[l]
    R.fill_(SENT)
    R[:end].fill_(-0.0)
    if n % 2:                                       # the odd batch's missing sample: stale, to be cleared
        R[T.HALO + T.SR * n: T.HALO + T.SR * n + T.L].fill_(STALE)
    ws.st[l].zero_()
    ctx = _ctx(ws, n, dropout, table=counters, counters=counters, seed=seed)
    return dict(ctx=ctx, a=a, amb=amb, l=l, n=n, mode=mode, dropout=dropout, seed=seed, tag=tag)


def _fwd_check(ws, S, M=1):
    a, amb, l, n, mode, dropout = (S[k] for k in ("a", "amb", "l", "n", "mode", "dropout"))
    R = ws.R[l]
    w, b = _p(ws, f"conv1d_{l + 1}/kernel"), _p(ws, f"conv1d_{l + 1}/bias")
    ref, allow, nw = T.fwd64(a, w, b, amb=amb)
    tag = f"fwd {l} n={n} {mode}" + ("" if dropout else " no-dropout") + (f" member {S['tag']} of {M}" if M > 1 else "")
    print(f"{tag}: {nw} of {ref.numel()} entries widened")
    out = T.take(R, n)
    _hold(tag + " |R|", out.abs(), ref, allow)
    drop = ~T.keep_mask(S["seed"], l, n, DEV) if dropout else torch.zeros_like(out, dtype=torch.bool)
    assert torch.equal(T.sign_bits(out), drop), tag + ": mask sign bits"
    assert bool((out[:, :, 0].abs() == 0).all()) and bool((out[:, :, 1].abs() == 0).all())
    _check_rows_outside(tag, R, n, SENT, NEG0)
    grid = T.geo(n, M, mode == "det")["blocks"][l]["fwd"]["grid"]
    m, am = T.fwd_moments(out.abs().double(), n, grid, l)
    _hold(tag + " moment slots", ws.st[l].view(T.SLOTS, 2, -1).sum(0), m, am)


# ================================================================================================ dgrad
def _bwd_fixture(ws, l, n, dropout, mode, seed=SEED, tag=0):
    """Block l's R_l, dY_l (or dlogit for block 6), its BN rows and backward means, as the mode delivers them
    (table rows the test wrote, or slots) -> float64 (mag, drop, dy, rows) the references take."""
    C = T.CH[l + 1]
    mag, drop = T.act_fixture(l, n, seed, dropout, tag)
    _put_R(ws, l, mag, drop, n)
    mag, drop = _dev(mag), drop.to(DEV)
    if l == 5:
        dlog = (torch.randn(n, generator=T._gen(26, n, tag)) / n).float()
        ws.dlogit.fill_(STALE)
        ws.dlogit[:n] = dlog.to(DEV)
        dy = T.head_dy64(drop, _dev(dlog), _p(ws, "output_layer/kernel"), T.dsc(5) if dropout else 1.0)
    else:
        dy = _dev(T.grad_fixture(l, n, seed, tag))
        _put_grad(ws.dY[l], dy, n)
    gamma, beta = _p(ws, f"batchnorm_{l + 1}/gamma"), _p(ws, f"batchnorm_{l + 1}/beta")
    st = T.moment_slots(mag)
    r0 = T.bn_rows64(st, 1.0 / (n * T.L), gamma, beta)
    xh = (mag - T.f32(r0["mean"])) * T.f32(r0["rstd"])
    tot = torch.stack([dy.sum((0, 1)), (dy * xh).sum((0, 1))])
    bst = torch.zeros(T.SLOTS, 2, C, dtype=torch.float64, device=DEV)
    bst[3], bst[11] = 0.25 * tot, 0.75 * tot
    _put_slots(ws.st[l], st)
    _put_slots(ws.bst[l], bst)
    return mag, drop, dy, st, bst


def _rows_of(ws, l, n, dropout, st, bst, mode, own_bwd, seed=SEED):
    """The fp32 rows the backward kernels use for block l.  'table': the test writes them (and the kernel
    reads them, except the backward means it sums itself with ``own_bwd``); 'slots': the kernel computes all
    of them from the slots -- taken here from what op 5 writes for the same slots."""
    tw = ws if ws.det is None else _ws(ws.B, False)
    if tw is not ws:
        _put_slots(tw.st[l], st)
        _put_slots(tw.bst[l], bst)
    ctx = _ctx(tw, n, dropout, seed=seed)
    _call(ctx, 5, 0, 0)
    _call(ctx, 5, l, 1)
    rows = {k: v.clone() for k, v in _tab_rows(tw, l).items()}
    if mode == "table" and not own_bwd:   # table means the kernel must READ: make them differ from the slots'
        rows["mdy"], rows["mdyx"] = T.f32(rows["mdy"] * 1.25), T.f32(rows["mdyx"] * 0.75)
        _put_tab(ws, l, mdy=rows["mdy"], mdyx=rows["mdyx"])
    return rows


DG_BIG = 1026      # 1026: 513 tiles on 512 persistent workgroups -- one runs two tiles, the rest one
DG_CASES = [(l, n, n, "table", True) for l in range(1, 6) for n in (1, 2, 37)] + \
           [(l, 3, 8, "table", True) for l in range(1, 6)] + [(l, DG_BIG, DG_BIG, "table", True) for l in range(1, 6)] + \
           [(l, 37, 37, m, True) for l in (1, 4, 5) for m in ("slots", "bwd_self", "det")] + \
           [(l, 37, 37, "fused", True) for l in (1, 4)] + [(2, 37, 37, "table", False), (5, 37, 37, "table", False)]


@pytest.mark.parametrize("l,n,n_alloc,mode,dropout", DG_CASES)
def test_dgrad_matches_float64(l, n, n_alloc, mode, dropout):
    """``dgrad_kernel<l>`` (op 2): the dZ_l it recomputes and stores (one bf16 store plus the fp32 operations
    of the BN backward), then dY_{l-1} against the transposed conv OF THE dZ_l THE KERNEL WROTE, exactly 0
    where block l-1 dropped, and the backward sums of block l-1 over the stored dY_{l-1}.  'table' / 'slots' /
    'det': where the BN rows come from; 'bwd_self': the backward means summed from the slots (flag bit 0);
    'fused': the launch also reduces wgrad<l+1>'s partial region (flag bit 1; that gradient is the wgrad
    test's), its own outputs unchanged."""
    g = T.geo(DG_BIG)           # one tile more than the persistent grid
    assert T.tiles(DG_BIG) == g["dg_grid"] + 1 == g["blocks"][1]["dgrad"]["grid"] + 1 and g["blocks"][1]["dgrad"]["persist"]
    ws = _ws(n_alloc, mode == "det")
    S = _dgrad_prepare(ws, l, n, mode, dropout)
    _call(S["ctx"], 2, l, {"bwd_self": 1, "fused": 2}.get(mode, 0))
    _dgrad_check(ws, S)


def _dgrad_prepare(ws, l, n, mode, dropout, seed=SEED, tag=0, counters=False):
    det = mode == "det"
    mag, drop, dy, st, bst = _bwd_fixture(ws, l, n, dropout, mode, seed, tag)
    tabled = mode in ("table", "bwd_self", "fused")
    own = l == 5 or mode not in ("table", "fused")
    rows = _rows_of(ws, l, n, dropout, st, bst, "table" if tabled else "slots", own, seed)
    magp, dropp = T.act_fixture(l - 1, n, seed, dropout, tag)
    _put_R(ws, l - 1, magp, dropp, n)
    magp, dropp = _dev(magp), dropp.to(DEV)
    stp = T.moment_slots(magp)
    _put_slots(ws.st[l - 1], stp)
    tw = ws if not det else _ws(ws.B, False)
    if det:
        _put_slots(tw.st[l - 1], stp)
    _call(_ctx(tw, n, dropout, seed=seed), 5, 0, 0)  # block l-1's mean / rstd (and block l's forward rows again)
    rp = {k: v.clone() for k, v in _tab_rows(tw, l - 1).items()}
    ctx = _ctx(ws, n, dropout, table=tabled, counters=counters, seed=seed)
    if tabled and not own:
        _put_tab(ws, l, mdy=rows["mdy"], mdyx=rows["mdyx"])
    for buf in (ws.dZ[l], ws.dY[l - 1]):     # (the 4 rows before the first tile are never written: zeros)
        buf.fill_(SENT)
        buf[: T.HALO].zero_()
    ws.bst[l - 1].zero_()
    return dict(ctx=ctx, mag=mag, dy=dy, rows=rows, magp=magp, dropp=dropp, rp=rp, l=l, n=n, mode=mode,
                dropout=dropout, tag=tag)


def _dgrad_check(ws, S, M=1):
    mag, dy, rows, magp, dropp, rp, l, n, mode, dropout = (
        S[k] for k in ("mag", "dy", "rows", "magp", "dropp", "rp", "l", "n", "mode", "dropout"))
    tag = f"dgrad {l} n={n} {mode}" + ("" if dropout else " no-dropout") + (f" member {S['tag']} of {M}" if M > 1 else "")
    dz, a_dz = T.dz64(mag, dy, rows["s"], rows["mean"], rows["rstd"], rows["mdy"], rows["mdyx"])
    dzs = T.take(ws.dZ[l], n)
    _hold(tag + " dZ", dzs, dz, a_dz + T.UB * dz.abs())
    _check_rows_outside(tag + " dZ", ws.dZ[l], n, SENT, 0)
    w = _p(ws, f"conv1d_{l + 1}/kernel")
    ref, al = T.dgrad64(dzs.double(), w, ~dropp, T.dsc(l - 1) if dropout else 1.0)
    dys = T.take(ws.dY[l - 1], n)
    _hold(tag + " dY", dys, ref, al)
    assert bool((dys[dropp] == 0).all()), tag + ": mask of block l-1"
    _check_rows_outside(tag + " dY", ws.dY[l - 1], n, SENT, 0)
    b, ab = T.bwd_sums64(dys.double(), magp, rp["mean"], rp["rstd"])
    _hold(tag + " bst[l-1]", ws.bst[l - 1].view(T.SLOTS, 2, -1).sum(0), b, ab)


# ================================================================================================ wgrad
WG_BIG = [2 * 1024 + 2, 2 * 1024]       # 1025 / 1024 row tiles: either side of the row-tile cap (tiles > 1024)
WG_CASES = [(l, n, n, "reduce", True) for l in range(6) for n in (1, 2, 37)] + \
           [(l, 3, 8, "reduce", True) for l in range(6)] + \
           [(l, n, n, "reduce", True) for l in range(6) for n in WG_BIG] + \
           [(l, 37, 37, m, True) for l in (0, 1, 3, 5) for m in ("fused", "atomic", "slots", "bwd_self")] + \
           [(0, 37, 37, "reduce", False), (4, 37, 37, "reduce", False)]


@pytest.mark.parametrize("l,n,n_alloc,mode,dropout", WG_CASES)
def test_wgrad_matches_float64(l, n, n_alloc, mode, dropout):
    """``wgrad_kernel<l>`` (op 3) with its reduction: dW_l, db_l from R_{l-1} (staged like the forward's input)
    and a dZ_l the test wrote -- block 1 forms dZ_0 itself from R_0 and dY_0.  'reduce': partial slots and
    the separate reduce launch, whose side job writes block l-1's backward table rows; 'fused': no reduce
    launch, the partials are reduced by dgrad<l-1> (l >= 2) or by the finalize launch (l <= 1); 'atomic': no
    partials; 'slots': no table; 'bwd_self': the backward means from the slots.  n = 37 gives row-group
    counts that are no multiple of the reduction's J."""
    assert T.wg(0, 37)["rgs"] % T.wg(0, 37)["J"] != 0 and T.wg(0, 37)["J"] > 1
    assert T.wg(4, WG_BIG[0])["rt"] > T.wg(4, 1)["rtiles"] >= T.wg(4, WG_BIG[1])["rt"]
    ws = _ws(n_alloc)
    S = _wgrad_prepare(ws, l, n, mode, dropout)
    ctx = S["ctx"]
    _call(ctx, 3, l, {"reduce": 0, "fused": 2, "atomic": 0, "slots": 0, "bwd_self": 1}[mode])
    if mode == "fused":
        if l >= 2:      # dgrad<l-1> reduces wgrad<l>'s partials (its own outputs are another test's)
            _call(ctx, 2, l - 1, 2)
        else:
            # the finalize launch reduces the regions of wgrad<1> and wgrad<0>: run the other one too (on
            # whatever its buffers hold: its gradient is another case's)
            _call(ctx, 3, 1 - l, 2)
            _call(ctx, 4, 0, 2)
    _wgrad_check(ws, S)


def _wgrad_prepare(ws, l, n, mode, dropout, seed=SEED, tag=0, counters=False):
    table = mode in ("reduce", "fused", "bwd_self")
    amb_dz, bstp = None, None
    if l == 0:
        mag, drop, dy, st, bst = _bwd_fixture(ws, 0, n, dropout, mode, seed, tag)
        rows = _rows_of(ws, 0, n, dropout, st, bst, "table" if table else "slots", mode not in ("reduce", "fused"), seed)
        a, amb = _fwd_inputs(ws, 0, n, dropout, seed, tag)
        dz, a_dz = T.dz64(mag, dy, rows["s"], rows["mean"], rows["rstd"], rows["mdy"], rows["mdyx"])
        dzb = T.bf(dz)
        # a dZ_0 within its fp32 allowance of a bf16 rounding boundary may round either way
        _, e = torch.frexp(dz.abs())
        ulp = torch.ldexp(torch.ones_like(dz), e - 8)
        dist = (torch.remainder(dz.abs() / ulp, 1.0) - 0.5).abs() * ulp
        amb_dz = torch.where((dist <= a_dz) & (mag > 0), ulp, torch.zeros_like(dz))
        dz = dzb
    else:
        a, amb = _fwd_inputs(ws, l, n, dropout, seed, tag)
        dz = _dev(T.grad_fixture(l, n, seed, tag=tag + 100))
        _put_grad(ws.dZ[l], dz, n)
        bstp = torch.randn(T.SLOTS, 2, T.CH[l], generator=T._gen(27, l, tag), dtype=torch.float64).to(DEV) * 1e-3
        _put_slots(ws.bst[l - 1], bstp)
        _put_slots(ws.st[l], T.moment_slots(_dev(T.act_fixture(l, n, seed, dropout, tag)[0])))
    ctx = _ctx(ws, n, dropout, table=table, wpart=mode != "atomic", counters=counters, seed=seed)
    ws.grad.fill_(0.0 if mode == "atomic" else SENT)     # atomics add into the gradient buffer
    if table and l > 0:
        tabv = ws.tab.view(6, T.TAB_ROWS, 256)
        tabv[l - 1, T.T_MDY:] = SENT
    return dict(ctx=ctx, a=a, amb=amb, dz=dz, amb_dz=amb_dz, bstp=bstp, l=l, n=n, mode=mode, dropout=dropout, tag=tag)


def _wgrad_check(ws, S, M=1):
    a, amb, dz, amb_dz, bstp, l, n, mode, dropout = (
        S[k] for k in ("a", "amb", "dz", "amb_dz", "bstp", "l", "n", "mode", "dropout"))
    gw, gb, a_gw, a_gb, nw = T.wgrad64(a, dz, l, n, M, amb=amb, amb_dz=amb_dz)
    tag = f"wgrad {l} n={n} {mode}" + ("" if dropout else " no-dropout") + (f" member {S['tag']} of {M}" if M > 1 else "")
    print(f"{tag}: {nw} of {gw.numel()} entries widened")
    _hold(tag + " dW", ws.gviews[f"conv1d_{l + 1}/kernel"], gw, a_gw)
    _hold(tag + " db", ws.gviews[f"conv1d_{l + 1}/bias"], gb, a_gb)
    if mode in ("reduce", "fused") and l > 0:   # the side job: block l-1's backward table rows
        ref, al = T.slot_mean64(bstp, 1.0 / (n * T.L))
        got = _tab_rows(ws, l - 1)
        _hold(tag + " table rows of block l-1", torch.stack([got["mdy"], got["mdyx"]]), ref, al)


# ================================================================================================ member-batched
MB_CASES = [(2, 16), (3, 5)]      # M = 2 at 16 samples: every grid.x * M is a multiple of 8 (the XCD remap of mb_pos)


@pytest.mark.parametrize("M,n", MB_CASES)
@pytest.mark.parametrize("kernel,l", [("fwd", 3), ("head", 5), ("dgrad", 4), ("wgrad", 5)])
def test_member_batched_matches_float64(kernel, l, M, n):
    """``train_args_dev`` + ``train_call_mb``: one launch over M members with different weights, inputs and
    dropout seeds, every member's outputs held to ITS OWN reference (a member reading another's Args fails).
    M = 2 with even workgroup counts takes the XCD remap of ``mb_pos``, M = 3 the fallback."""
    if M == 2:   # grid.x of fwd (tiles), head (n / 4), dgrad (tiles), wgrad (blocks x row groups): all x 2 = 0 mod 8
        g = T.geo(n, M)
        grids = (g["blocks"][3]["fwd"]["grid"], g["head"]["grid"], g["blocks"][4]["dgrad"]["grid"], g["blocks"][5]["wgrad"]["grid"])
        assert grids[:2] == (T.tiles(n), n // 4)
        assert all((g * M) % 8 == 0 for g in grids)
    prepare, check, op, flag = {"fwd": (_fwd_prepare, _fwd_check, 0, 0), "head": (None, _head_check, 1, 1),
                                "dgrad": (_dgrad_prepare, _dgrad_check, 2, 0),
                                "wgrad": (_wgrad_prepare, _wgrad_check, 3, 0)}[kernel]
    wss = [_ws(n, False, 3 + m) for m in range(M)]
    states = []
    for m, ws in enumerate(wss):
        ws.counters[0] = T.PASS - train_ops.TRAIN_PASS_BASE     # the device step counter the masks are keyed by
        if kernel == "head":
            states.append(_head_prepare(ws, n, "table", 0.25 + m, True, SEED + m, m, True))
        else:
            states.append(prepare(ws, l, n, "atomic" if kernel == "fwd" else "table" if kernel == "dgrad" else "reduce",
                                  True, SEED + m, m, True))
    o = _ext.ops()
    args = o.train_args_dev([s["ctx"] for s in states], 0)
    o.train_call_mb(args, states[0]["ctx"], M, op, l, flag)
    for ws, s in zip(wss, states):
        check(ws, s, M)
        ws.counters.zero_()
