"""GPU numerics of the layer-wise HIP training kernels vs fp32 autograd over the reference ops."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.cnn import AlarconCNN1D
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, train_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.training.step import TRAIN_PASS_BASE

from .train_emulation import emulate_step

pytestmark = pytest.mark.gpu


def _torch_grads(model, x, y):
    store = model.store
    flat = store.flat.detach().clone().requires_grad_(True)
    stats = store.stats.detach().clone()
    p = {}
    for n in store.trainable:
        off = store.offsets[n]
        p[n] = flat[off: off + store.views[n].numel()].view(store.shapes[n])
    off = 0
    for n in store.nontrainable:
        k = store.views[n].numel()
        p[n] = stats[off: off + k].view(store.shapes[n])
        off += k
    logits = R.forward(model.spec, p, x, dropout=True, bn_batch_stats=True, update_moving=True, seed=model.seed,
                       pass_id=TRAIN_PASS_BASE + model._train_step_counter, sample_ids=torch.arange(x.shape[0], device=x.device),
                       return_logits=True)
    lv = torch.nn.functional.binary_cross_entropy_with_logits(logits.reshape(-1), y, reduction="none")
    lv.mean().backward()
    return lv.sum().item(), flat.grad.detach(), stats, logits.detach().reshape(-1)


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# 2563: 1282 row tiles, so the persistent dgrad workgroups (at most 512) run 2-3 tiles each with the
# next tile's staging prefetched, and the 8-wave wgrad several row tiles per workgroup; odd: a half tile
@pytest.mark.parametrize("n", [64, 37, 2563])
def test_hip_train_step_matches_autograd(n):
    _ext.require()
    dev = torch.device("cuda")
    m = AlarconCNN1D(seed=5, device=dev)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 60, 4, generator=g).to(dev)
    y = (torch.rand(n, generator=g) > 0.5).float().to(dev)
    m.optimizer.learning_rate = 0.0
    p0 = {k: v.clone() for k, v in m.store.as_dict().items()}
    ref_loss, ref_grad, ref_stats, ref_logits = _torch_grads(m, x, y)
    em_loss, em_logits, em_grad, em_stats = emulate_step(m.spec, p0, x, y, m.seed, TRAIN_PASS_BASE)
    loss, probs = train_ops.train_step(m, x, y)
    ws = m._train_ws
    assert abs(loss.item() - ref_loss) / ref_loss < 2e-2
    assert abs(loss.item() - em_loss) / em_loss < 2e-3
    torch.testing.assert_close(ws.logits[:n], ref_logits, atol=5e-2, rtol=5e-2)
    st = m.store
    for name in st.trainable:
        off, k = st.offsets[name], st.views[name].numel()
        hip = ws.grad[off: off + k]
        # tight vs the bf16-dataflow emulation, direction-only vs fp32 autograd (BN-backward
        # cancellation turns bf16 quantisation into ~10-20 % relative noise, see train_emulation.py)
        e = _rel(hip, em_grad[name].reshape(-1))
        print(f"[step n={n}] {name}: {e:.4f}")
        assert e < 0.12, (name, e)
        cos = torch.nn.functional.cosine_similarity(hip, ref_grad[off: off + k], dim=0).item()
        assert cos > 0.97, (name, cos)
    for name, v in em_stats.items():
        torch.testing.assert_close(st.views[name], v, atol=2e-3, rtol=2e-2)


@pytest.mark.parametrize("n,max_samples", [(50, 1 << 20), (37, 80), (2049, 1 << 20), (2051, 4200)])
def test_batch_stats_mc_dropout_matches_reference(n, max_samples):
    """bf16 engine (the fp32-faithful one: tests/test_x3_gpu.py).  Odd n: tiles straddle pass
    boundaries; max_samples=80 / 4200: several pass chunks share block 1's output and moments.  The
    bound is set from the measured bf16 deviation (max |dp| 4.1e-3 at T=50 x 1024 windows, BENCH_r02)."""
    _ext.require()
    dev = torch.device("cuda")
    m = AlarconCNN1D(seed=6, device=dev)
    x = torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(0)).to(dev)
    snap = m.snapshot()
    got = train_ops.forward_batch_stats(m, x, 3, pass_base=0, seed=m.seed, update_moving=True,
                                        max_samples=max_samples)
    hip_stats = m.store.stats.clone()
    m.restore(snap)
    ref = []
    for t in range(3):
        ref.append(torch.sigmoid(R.forward(m.spec, m.store.as_dict(), x, dropout=True, bn_batch_stats=True,
                                           update_moving=True, seed=m.seed, pass_id=t, return_logits=True)).reshape(-1))
    ref = torch.stack(ref)
    torch.testing.assert_close(got, ref, atol=1e-2, rtol=0)
    torch.testing.assert_close(hip_stats, m.store.stats, atol=2e-3, rtol=2e-2)


def test_batch_bn_moments_fp64_at_bench_scale():
    """BN batch moments over 16384 windows x 60 rows per channel (the reference's whole-test-set
    batch, uq_techniques.py:22) vs fp64 moments of the very activations the kernels stored."""
    _ext.require()
    dev = torch.device("cuda")
    m = AlarconCNN1D(seed=7, device=dev)
    n = 16384
    x = torch.randn(n, 60, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    train_ops.forward_batch_stats(m, x, 1, pass_base=0, seed=m.seed, update_moving=False, max_samples=n)
    ws = m._mcd_ws
    for l in range(6):
        c = ws.ch[l + 1]
        r = ws.R[l][train_ops.HALO: train_ops.HALO + train_ops.SR * n].view(n, train_ops.SR, c)[:, :60]
        v = (r.view(torch.int16) & 0x7FFF).view(torch.bfloat16).double().reshape(-1, c)  # |R|: sign = dropout mask
        mu_ref, var_ref = v.mean(0), v.var(0, unbiased=False)
        st = ws.st[l].view(train_ops.STAT_SLOTS, ws.groups, 2, c)[:, 0].sum(0)
        mu = st[0] / (n * 60)
        var = st[1] / (n * 60) - mu * mu
        assert ((mu - mu_ref).abs() / mu_ref.abs().clamp_min(1e-3)).max().item() < 1e-5, l
        assert ((var - var_ref).abs() / var_ref.clamp_min(1e-6)).max().item() < 1e-5, l


def test_hip_training_reduces_loss():
    _ext.require()
    from uncertaintyquantification_sleepapnea_1dcnn_amd.data.synthetic import synthetic_windows

    x, y, _ = synthetic_windows(2048, seed=1)
    m = AlarconCNN1D(seed=1, device="cuda")
    h = m.fit(x, y.astype(np.float32), batch_size=256, epochs=3, validation_split=0.1, verbose=0)
    assert h.history["loss"][-1] < h.history["loss"][0]
    assert h.history["val_accuracy"][-1] > 0.8


def _four_steps(monkeypatch, graph, x, y):
    monkeypatch.setenv("APNEAUQ_TRAIN_GRAPH", graph)
    m = AlarconCNN1D(seed=3, device="cuda")
    losses = [float(m.train_step(x[i * 64:(i + 1) * 64], y[i * 64:(i + 1) * 64])) for i in range(4)]
    if graph == "1":
        assert 64 in getattr(m, "_train_graphs", {})  # the graph path really ran
    return losses, m.store.flat.clone(), m.store.stats.clone(), (m.optimizer.iterations, m._train_step_counter)


def test_graphed_training_step_matches_eager(monkeypatch, deterministic):
    """The HIP-graph replay of the training step (device-side dropout pass / Adam step counters)
    IS the eager HIP step: in deterministic mode 4 steps give bitwise-identical losses, weights and
    BN statistics.  In atomic mode only step 1 is compared (identical weights, masks and inputs):
    later steps inherit the fp32 summation order of the atomics."""
    from uncertaintyquantification_sleepapnea_1dcnn_amd.data.synthetic import synthetic_windows

    x, y, _ = synthetic_windows(256, seed=5)
    x = torch.as_tensor(x, dtype=torch.float32).cuda()
    y = torch.as_tensor(y, dtype=torch.float32).cuda()
    le, we, se, ce = _four_steps(monkeypatch, "0", x, y)
    lg, wg, sg, cg = _four_steps(monkeypatch, "1", x, y)
    assert ce == cg == (4, 4)
    assert lg == le
    assert torch.equal(wg, we) and torch.equal(sg, se)
    train_ops.set_deterministic(False)
    la, _, _, _ = _four_steps(monkeypatch, "0", x, y)
    lb, _, _, _ = _four_steps(monkeypatch, "1", x, y)
    assert abs(lb[0] - la[0]) < 1e-4 * abs(la[0])


def test_graphed_step_overlap_matches_single_stream(monkeypatch):
    """The graphed step with the wgrad chain on its own captured stream (train_ops.OVERLAP) computes
    the gradients of the one-stream graph: same loss and, up to the atomics' summation order, the
    same gradient of every parameter (the backward BN rows are summed from the same fp64 slots either
    way).  The atomic mode's order noise moves single near-zero elements through bf16 rounding (seen:
    3.7e-5 absolute), so each tensor is compared by its relative L2 error; a missing fork / join
    edge would leave a whole tensor stale or half-summed (O(1) error)."""
    from uncertaintyquantification_sleepapnea_1dcnn_amd.data.synthetic import synthetic_windows

    x, y, _ = synthetic_windows(512, seed=9)
    x = torch.as_tensor(x, dtype=torch.float32).cuda()
    y = torch.as_tensor(y, dtype=torch.float32).cuda()
    monkeypatch.setenv("APNEAUQ_TRAIN_GRAPH", "1")
    train_ops.set_deterministic(False)
    out = {}
    for ov in (False, True):
        monkeypatch.setattr(train_ops, "OVERLAP", ov)
        m = AlarconCNN1D(seed=4, device="cuda")
        loss = float(m.train_step(x, y))
        step = m._train_graphs[512]
        assert step.overlap == ov
        out[ov] = (loss, {k: v.clone() for k, v in step.ws.gviews.items()})
    assert abs(out[True][0] - out[False][0]) <= 1e-5 * abs(out[False][0])
    for name, g0 in out[False][1].items():
        g1 = out[True][1][name]
        assert torch.isfinite(g1).all(), name
        rel = ((g1 - g0).norm() / g0.norm().clamp_min(1e-30)).item()
        assert rel < 5e-3, (name, rel)


@pytest.mark.parametrize("graph,batch", [("1", 512), ("0", 384), ("1", 4100)])
def test_fused_reductions_match_separate_launches(monkeypatch, graph, batch):
    """The fused step (train_ops.FUSED_REDUCE: wgrad_l's partials reduced inside dgrad_{l-1}, those of
    wgrad_1 / wgrad_0 next to the BN finalize, the table's backward rows written by wgrad's workgroup 0)
    computes the separate launches' step: same loss and every gradient tensor within the atomics' order
    noise (a skipped or misplaced reduction leaves a tensor stale or zero: O(1) error).  Step 2 runs
    from identical states (the fused model gets the other's weights, statistics and Adam moments) so a
    table row left stale from step 1 would show.  (Without the copy, Adam's ~lr first moves of
    near-zero gradient elements whose sign the order noise flips move block 1's step-2 gradient by up to
    7 %.)  Batch 4100 runs the large-batch row grouping and a partial last row tile; the eager case adds a
    100-sample step on the 384-sample workspace."""
    from uncertaintyquantification_sleepapnea_1dcnn_amd.data.synthetic import synthetic_windows

    x, y, _ = synthetic_windows(batch, seed=11)
    x = torch.as_tensor(x, dtype=torch.float32).cuda()
    y = torch.as_tensor(y, dtype=torch.float32).cuda()
    monkeypatch.setenv("APNEAUQ_TRAIN_GRAPH", graph)
    monkeypatch.setattr(train_ops, "FUSED_MAX_BATCH", 1 << 20)
    train_ops.set_deterministic(False)
    models, losses, grads = {}, {}, {}

    def step(fused):
        monkeypatch.setattr(train_ops, "FUSED_REDUCE", fused)
        m = models[fused]
        losses.setdefault(fused, []).append(float(m.train_step(x, y)))
        ws = m._train_graphs[batch].ws if graph == "1" else m._train_ws
        assert train_ops._fused(ws, x.shape[0]) == fused
        grads.setdefault(fused, []).append({k: v.clone() for k, v in ws.gviews.items()})

    for fused in (False, True):
        models[fused] = AlarconCNN1D(seed=6, device="cuda")
        step(fused)
    a, b = models[False], models[True]
    b.store.flat.copy_(a.store.flat)
    b.store.stats.copy_(a.store.stats)
    b.optimizer.m.copy_(a.optimizer.m)
    b.optimizer.v.copy_(a.optimizer.v)
    for fused in (False, True):
        step(fused)
    nsteps = 2
    if graph == "0":  # eager: a partial batch on the same workspace (n < capacity: its own row grouping)
        b.store.flat.copy_(a.store.flat)
        b.store.stats.copy_(a.store.stats)
        b.optimizer.m.copy_(a.optimizer.m)
        b.optimizer.v.copy_(a.optimizer.v)
        x, y = x[:100], y[:100]
        for fused in (False, True):
            step(fused)
        nsteps = 3
    for i in range(nsteps):
        assert abs(losses[True][i] - losses[False][i]) <= 1e-5 * abs(losses[False][i]), (i, losses)
        for name, g0 in grads[False][i].items():
            g1 = grads[True][i][name]
            assert torch.isfinite(g1).all(), name
            rel = ((g1 - g0).norm() / g0.norm().clamp_min(1e-30)).item()
            assert rel < 5e-3, (i, name, rel)


def test_fit_concurrent_on_streams_matches_sequential(deterministic):
    """Three members trained concurrently (training/trainer.py:fit_concurrent), on HIP streams and as
    member-batched launches, ARE back-to-back fits in deterministic mode (bitwise-identical loss
    histories and weights), and train_ensemble on one GPU uses the concurrent path."""
    import os
    import tempfile

    from uncertaintyquantification_sleepapnea_1dcnn_amd.parallel.ensemble import load_ensemble_prefix, train_ensemble
    from uncertaintyquantification_sleepapnea_1dcnn_amd.training.trainer import fit_concurrent

    g = torch.Generator().manual_seed(2)
    x = torch.randn(3072, 60, 4, generator=g)
    y = (x[:, :, 0].mean(1) > 0).float()
    kw = dict(epochs=3, batch_size=512, validation_split=0.1, verbose=0)
    seq = [AlarconCNN1D(seed=20 + i, device="cuda") for i in range(3)]
    h_seq = [m.fit(x, y, **kw) for m in seq]
    for batched in (False, True):
        con = [AlarconCNN1D(seed=20 + i, device="cuda") for i in range(3)]
        h_con = fit_concurrent(con, x, y, batched=batched, **kw)
        for hs, hc, ms, mc in zip(h_seq, h_con, seq, con):
            assert hc.history["loss"] == hs.history["loss"], (batched, hc.history["loss"], hs.history["loss"])
            assert torch.equal(mc.store.flat, ms.store.flat), batched
    with tempfile.TemporaryDirectory() as d:
        paths = train_ensemble(x.numpy(), y.numpy(), num_models=3, save_dir=d, prefix="m", name_offset=0, epochs=2,
                               batch_size=512, verbose=0, epoch_backup=False)
        assert all(os.path.exists(p) for p in paths)
        assert len(load_ensemble_prefix(os.path.join(d, "m"), 3, device="cuda")) == 3


def test_bf16_hip_training_matches_fp32_training(monkeypatch, deterministic):
    """bf16 HIP training tracks fp32 training: same data, seed and Keras loop (10 epochs,
    batch 1024, validation_split=0.1 -> tail slice).  Every epoch's training loss agrees within 2 %
    and the best val AUC within 0.01.  (Val LOSS is not compared: on the tail slice it is evaluated
    with Keras moving-average BN statistics that lag the weights, and swings 0.1 <-> 1.1 from epoch to
    epoch in BOTH backends -- tools/probes/parity_train.py, profiles/train_parity_r2.jsonl.)  The
    windows are the synthetic apnea set with extra noise so the task is not saturated."""
    _ext.require()
    from uncertaintyquantification_sleepapnea_1dcnn_amd.data.synthetic import synthetic_windows

    x, y, _ = synthetic_windows(32768, seed=2025)
    rs = np.random.RandomState(2025)
    x = (x + rs.randn(*x.shape).astype(np.float32) * 1.6).astype(np.float32)
    x = (x - x.mean(1, keepdims=True)) / (x.std(1, keepdims=True) + 1e-8)
    res = {}
    for backend in ("hip", "torch"):
        monkeypatch.setenv("APNEAUQ_TRAIN_BACKEND", backend)
        m = AlarconCNN1D(seed=2025, device="cuda")
        res[backend] = m.fit(x, y.astype(np.float32), batch_size=1024, epochs=10, validation_split=0.1,
                             verbose=0).history
    hh, ht = res["hip"], res["torch"]
    # 2 % relative, plus 2e-3 absolute for the late epochs (loss ~0.06), where bf16 rounding alone moves
    # the loss by ~1e-3 (r2 session 3: 0.0012 = 2.05 % at epoch 8; deterministic mode: reproducible)
    np.testing.assert_allclose(hh["loss"], ht["loss"], rtol=0.02, atol=2e-3)
    assert 0.9 < ht["val_auc"][-1] < 0.9999, ht["val_auc"]
    # val AUC on the tail slice swings by a few 1e-2 from epoch to epoch in BOTH backends (moving-average
    # BN statistics, as for val loss): the best epoch must agree to 0.01, the last one to 0.05 (r2 s3:
    # best 0.9919 vs 0.9926, last 0.949 vs 0.936)
    assert abs(max(hh["val_auc"]) - max(ht["val_auc"])) < 0.01, (hh["val_auc"], ht["val_auc"])
    assert abs(hh["val_auc"][-1] - ht["val_auc"][-1]) < 0.05, (hh["val_auc"], ht["val_auc"])


def _member_steps(x, y, batched: bool):
    ms = [AlarconCNN1D(seed=10 + i, device="cuda") for i in range(3)]
    ls = [[], [], []]
    b = x.shape[2]
    if batched:
        st = train_ops.GraphedEnsembleStep(ms, b)
        for s in range(4):
            out = st([x[i, s] for i in range(3)], [y[i, s] for i in range(3)])
            for i, (loss, p) in enumerate(out):
                ls[i].append(float(loss))
                assert p.shape == (b,) and bool(((p > 0) & (p < 1)).all())
    else:
        ls = [[float(m.train_step(x[i, s], y[i, s])) for s in range(4)] for i, m in enumerate(ms)]
    return ms, ls


# batch 1100: 550 row tiles per member, so the member-batched persistent dgrad (512 / 3 workgroups per
# member) and the single-model one (512) loop over different tile sets per workgroup
@pytest.mark.parametrize("batch", [64, 1100])
def test_member_batched_step_matches_single_graphs(deterministic, batch):
    """GraphedEnsembleStep (one member-batched launch per layer for 3 members) IS each member's own
    graphed step: in deterministic mode 4 steps on member-specific batches give bitwise-identical
    losses, weights and BN statistics, and the host / device counters advance alike.  Atomic mode:
    the first-step losses agree (later steps inherit the atomics' summation order)."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 4, batch, 60, 4, generator=g).cuda()
    y = (torch.rand(3, 4, batch, generator=g) < 0.4).float().cuda()
    single, ls = _member_steps(x, y, False)
    batched, lb = _member_steps(x, y, True)
    for i in range(3):
        assert (batched[i].optimizer.iterations, batched[i]._train_step_counter) == (4, 4)
        assert lb[i] == ls[i], (i, lb[i], ls[i])
        assert torch.equal(batched[i].store.flat, single[i].store.flat), i
        assert torch.equal(batched[i].store.stats, single[i].store.stats), i
    # members stay independent: member 1 with another seed's weights differs from member 0
    assert abs(lb[0][0] - lb[1][0]) > 1e-3
    train_ops.set_deterministic(False)
    _, la = _member_steps(x, y, False)
    _, lc = _member_steps(x, y, True)
    for i in range(3):
        assert abs(lc[i][0] - la[i][0]) < 1e-4 * abs(la[i][0])


def test_fit_concurrent_batched_matches_streams(deterministic):
    """fit_concurrent's member-batched mode (one GraphedEnsembleStep per round, tail batches and
    members that stop early included) equals the stream mode epoch by epoch, bitwise in
    deterministic mode."""
    from uncertaintyquantification_sleepapnea_1dcnn_amd.training.callbacks import EarlyStopping
    from uncertaintyquantification_sleepapnea_1dcnn_amd.training.trainer import fit_concurrent

    g = torch.Generator().manual_seed(4)
    x = torch.randn(1100, 60, 4, generator=g)
    y = (x[:, :, 0].mean(1) > 0).float()
    hs, ws = {}, {}
    for mode in (False, True):
        ms = [AlarconCNN1D(seed=30 + i, device="cuda") for i in range(3)]
        cbs = [[EarlyStopping(monitor="loss", patience=0, min_delta=10.0)] if i == 2 else [] for i in range(3)]
        hs[mode] = fit_concurrent(ms, x, y, batched=mode, batch_size=256, epochs=3, verbose=0, shuffle=True,
                                  callbacks=cbs)
        ws[mode] = [m.store.flat.clone() for m in ms]
    for a, b, wa, wb in zip(hs[False], hs[True], ws[False], ws[True]):
        assert a.history["loss"] == b.history["loss"], (a.history["loss"], b.history["loss"])
        assert torch.equal(wa, wb)
    assert len(hs[True][2].history["loss"]) < 3  # the early-stopped member left the batched rounds


def test_member_batched_step_many_members():
    """17 members (beyond one zero / Adam launch; no XCD-aligned placement): every member's first-step
    loss equals its own graphed single-model step."""
    _ext.require()
    g = torch.Generator().manual_seed(9)
    M = 17
    x = torch.randn(M, 32, 60, 4, generator=g).cuda()
    y = (torch.rand(M, 32, generator=g) < 0.5).float().cuda()
    ref = [float(AlarconCNN1D(seed=40 + i, device="cuda").train_step(x[i], y[i])) for i in (0, 8, 16)]
    ms = [AlarconCNN1D(seed=40 + i, device="cuda") for i in range(M)]
    st = train_ops.GraphedEnsembleStep(ms, 32)
    out = st([x[i] for i in range(M)], [y[i] for i in range(M)])
    got = [float(out[i][0]) for i in (0, 8, 16)]
    np.testing.assert_allclose(got, ref, rtol=1e-4)
    out = st([x[i] for i in range(M)], [y[i] for i in range(M)])
    assert all(m.optimizer.iterations == 2 and m._train_step_counter == 2 for m in ms)
    assert all(np.isfinite(float(o[0])) for o in out)


def test_step_node_kernels():
    """The merged small nodes of the graphed step (round 5): ``train_inputs`` copies every member's x into
    the padded-row bf16 layout exactly as ``copy_`` does (round to nearest even, pad rows untouched) and y
    verbatim; ``train_tail`` bumps the counters once and writes sigmoid(logits) within 2 ulp of torch;
    ``gt_pack_zero`` packs like ``gt_pack`` and clears the listed buffers."""
    _ext.require()
    o = _ext.ops()
    g = torch.Generator().manual_seed(3)
    n, SR = 37, train_ops.SR
    xs = [torch.randn(n, 60, 4, generator=g).cuda() for _ in range(3)]
    ys = [torch.rand(n, generator=g).cuda() for _ in range(3)]
    xd = [torch.full((n * SR + 8, 4), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    yd = [torch.zeros(n + 5, device="cuda") for _ in range(3)]
    o.train_inputs(xs, ys, xd, yd, SR)
    for x, y, a, b in zip(xs, ys, xd, yd):
        v = a[: n * SR].view(n, SR, 4)
        assert torch.equal(v[:, :60], x.to(torch.bfloat16))
        assert bool((v[:, 60:] == 7.0).all()) and bool((a[n * SR:] == 7.0).all())
        assert torch.equal(b[:n], y) and bool((b[n:] == 0).all())
    cnt = torch.tensor([[3, 5], [7, 11]], dtype=torch.int32, device="cuda")
    lg = [torch.randn(n, generator=g).cuda() * 8 for _ in range(2)]
    pr = [torch.empty(n, device="cuda") for _ in range(2)]
    o.train_tail(cnt.view(-1), lg, pr)
    assert cnt.cpu().tolist() == [[4, 6], [8, 12]]
    for a, b in zip(lg, pr):
        torch.testing.assert_close(b, torch.sigmoid(a), rtol=2.5e-7, atol=1e-7)
    m = AlarconCNN1D(seed=4, device="cuda")
    ws = train_ops.TrainWorkspace(m, 64)
    for t in ws.accumulators():
        t.fill_(1)
    ws.pack()
    ref = [w.clone() for w in ws.wf] + [w.clone() for w in ws.wd[1:]]
    for w in ws.wf + ws.wd[1:]:
        w.zero_()
    ws.pack_zero()
    assert all(torch.equal(a, b) for a, b in zip(ref, list(ws.wf) + list(ws.wd[1:])))
    assert all(bool((t == 0).all()) for t in ws.accumulators())


def test_large_batch_prefetch_paths_match_deterministic(deterministic):
    """Batch 3000 (1500 row tiles): the atomic-mode step runs the prefetching persistent forward (FwdPF,
    512 workgroups over tile ranges), the deterministic one the plain one-tile-per-workgroup forward; both
    run the persistent dgrad and the 8-wave wgrad.  Same weights, masks and inputs: the same loss and
    gradients up to the summation order of the atomics."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(30)
    x = torch.randn(3000, 60, 4, generator=g).to(dev)
    y = (torch.rand(3000, generator=g) > 0.5).float().to(dev)
    out = {}
    for det in (True, False):
        train_ops.set_deterministic(det)
        m = AlarconCNN1D(seed=6, device=dev)
        m.optimizer.learning_rate = 0.0
        loss, _ = train_ops.train_step(m, x, y)
        out[det] = (float(loss), m._train_ws.grad.clone())
    (ld, gd), (la, ga) = out[True], out[False]
    assert abs(la - ld) < 1e-4 * abs(ld), (la, ld)
    assert _rel(ga, gd) < 1e-2, _rel(ga, gd)
    assert torch.nn.functional.cosine_similarity(ga, gd, dim=0).item() > 0.9999
