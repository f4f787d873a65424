"""GPU numerics of the generic HIP training path (``ops/generic_train.py``: ``csrc/generic_train.hip``
+ the kTrain / kLinear modes of ``csrc/generic_conv.hip``) for non-reference architectures -- pooled
blocks, the 30 s single-channel window, odd filter counts and kernel size 1 -- against fp32 autograd
over the reference ops with the same dropout masks; plus data-parallel (SyncBN) steps on 2 ranks
sharing the GPU against the single-process step, for this path and the reference architecture's.

These are whole-step bounds (a few percent on a gradient).  The tight ones -- every kernel of this path on its
own against float64, per entry -- are in ``test_generic_train_kernels_gpu.py``."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.models import reference as R
from uncertaintyquantification_sleepapnea_1dcnn_amd.models.cnn import AlarconCNN1D
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext, bn_batch, generic_train, train_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.training import step as tstep

from .dist_utils import run_ranks
from .generic_train_emulation import emulate_generic_step
from .test_generic_gpu import SPECS
from .test_train_gpu import _rel, _torch_grads

pytestmark = pytest.mark.gpu


def _batch(spec, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, spec.input_length, spec.input_channels, generator=g)
    y = (torch.rand(n, generator=g) > 0.5).float()
    return x.cuda(), y.cuda()


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("n", [64, 37])
def test_generic_train_step_matches_autograd(name, n):
    _ext.require()
    spec = SPECS[name]
    m = AlarconCNN1D(spec=spec, seed=5, device="cuda")
    assert tstep._backend(m) == "hip_generic"
    x, y = _batch(spec, n, n)
    m.optimizer.learning_rate = 0.0
    p0 = {k: v.clone() for k, v in m.store.as_dict().items()}
    ref_loss, ref_grad, ref_stats, _ = _torch_grads(m, x, y)
    em_loss, _, em_grad, em_stats = emulate_generic_step(spec, p0, x, y, m.seed, tstep.TRAIN_PASS_BASE)
    loss, probs = generic_train.train_step(m, x, y)
    ws = m._gtrain_ws
    assert abs(loss.item() - ref_loss) / ref_loss < 2e-2
    assert abs(loss.item() - em_loss) / em_loss < 2e-3
    st = m.store
    bad = []
    for nm in st.trainable:
        off, k = st.offsets[nm], st.views[nm].numel()
        hip, ref = ws.grad[off: off + k], ref_grad[off: off + k]
        # tight vs the bf16-dataflow emulation; direction-only vs fp32 autograd.  The BN backward
        # amplifies bf16 quantisation (a 1-ulp flip of a stored z where the MFMA and host summation
        # orders round differently); conv biases are pure cancellation residuals of dz (sum over
        # rows of a zero-mean quantity, and block 6 of the pooled spec normalises over L = 1),
        # hence the looser bounds for them
        cb = nm.startswith("conv") and nm.endswith("/bias")
        e = _rel(hip, em_grad[nm].reshape(-1))
        cos = torch.nn.functional.cosine_similarity(hip, ref, dim=0).item()
        if e > (0.25 if cb else 0.12) or cos < (0.9 if cb else 0.95):
            bad.append((nm, round(e, 4), round(cos, 4)))
    assert not bad, bad
    for nm, v in em_stats.items():
        torch.testing.assert_close(st.views[nm], v, atol=2e-3, rtol=2e-2)
    torch.testing.assert_close(st.stats, ref_stats, atol=3e-3, rtol=3e-2)


@pytest.mark.parametrize("name", ["pooled", "single30"])
def test_generic_fit_reduces_loss(name):
    """A few hundred steps on a learnable synthetic rule through the public fit() on the HIP path."""
    _ext.require()
    spec = SPECS[name]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2048, spec.input_length, spec.input_channels, generator=g)
    y = (x[:, :, 0].mean(1) > 0).float()
    m = AlarconCNN1D(spec=spec, seed=1, device="cuda")
    h = m.fit(x.numpy(), y.numpy(), batch_size=256, epochs=6, verbose=0)
    losses = h.history["loss"]
    assert losses[-1] < 0.8 * losses[0], losses


@pytest.mark.parametrize("name", ["pooled", "odd"])
def test_generic_batch_bn_mc_dropout_matches_reference(name, deterministic):
    """bf16 kernels (the fp32 default: tests/test_fp32_gpu.py)."""
    _ext.require()
    spec = SPECS[name]
    m = AlarconCNN1D(spec=spec, seed=6, device="cuda", precision="bf16")
    x, _ = _batch(spec, 50, 0)
    snap = m.snapshot()
    got = generic_train.forward_batch_stats(m, x, 3, pass_base=0, seed=m.seed, update_moving=True)
    hip_stats = m.store.stats.clone()
    m.restore(snap)
    ref = []
    for t in range(3):
        lg = R.forward(spec, m.store.as_dict(), x, dropout=True, bn_batch_stats=True, update_moving=True,
                       seed=m.seed, pass_id=t, sample_ids=torch.arange(50, device=x.device), return_logits=True)
        ref.append(torch.sigmoid(lg).reshape(-1))
    torch.testing.assert_close(got, torch.stack(ref), atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(hip_stats, m.store.stats, atol=3e-3, rtol=3e-2)
    # the public batch-BN MC Dropout dispatches here (no PyTorch fallback)
    m.restore(snap)
    out = bn_batch.mc_dropout_batch_bn(m, x, 3, seed=m.seed)
    assert torch.equal(out[..., 0], got)  # deterministic moment slots: the same kernels, the same bits


def _dp_grads(rank, world, name):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.parallel.data_parallel import DPContext

    spec = SPECS.get(name)
    m = AlarconCNN1D(spec=spec, seed=9, device="cuda") if spec is not None else AlarconCNN1D(seed=9, device="cuda")
    x, y = _batch(m.spec, 64, 1)
    parts = torch.tensor_split(torch.arange(64), world)
    off = sum(len(p) for p in parts[:rank])
    idx = parts[rank].cuda()
    m.dp = DPContext(None, world, rank)
    m.optimizer.learning_rate = 0.0
    tstep.train_step(m, x[idx], y[idx], dp_step=(64, off))
    ws = m._gtrain_ws if spec is not None else m._train_ws
    return ws.grad.cpu(), m.store.stats.cpu()


@pytest.mark.parametrize("name", ["pooled", "reference"])
def test_data_parallel_hip_step_matches_single_process(name):
    """SyncBN + one gradient bucket over 2 ranks == the single-device full-batch step."""
    _ext.require()
    res = run_ranks(_dp_grads, 2, (name,), gpu=True)
    spec = SPECS.get(name)
    m = AlarconCNN1D(spec=spec, seed=9, device="cuda") if spec is not None else AlarconCNN1D(seed=9, device="cuda")
    x, y = _batch(m.spec, 64, 1)
    m.optimizer.learning_rate = 0.0
    if spec is not None:
        generic_train.train_step(m, x, y)
        ref = m._gtrain_ws.grad.cpu()
    else:
        train_ops.train_step(m, x, y)
        ref = m._train_ws.grad.cpu()
    st = m.store
    for grad, stats in res:
        for nm in st.trainable:
            off, k = st.offsets[nm], st.views[nm].numel()
            e = _rel(grad[off: off + k], ref[off: off + k])
            assert e < 3e-2, (nm, e)
        torch.testing.assert_close(stats, st.stats.cpu(), atol=2e-3, rtol=2e-2)


def _generic_steps(monkeypatch, spec, graph, x, y):
    from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import generic_train, rng

    monkeypatch.setenv("APNEAUQ_TRAIN_GRAPH", graph)
    m = AlarconCNN1D(spec=spec, seed=4, device="cuda")
    losses = [float(m.train_step(x[i * 64:(i + 1) * 64], y[i * 64:(i + 1) * 64])) for i in range(4)]
    if graph == "1":
        gs = getattr(m, "_gtrain_graphs", {})
        assert 64 in gs
        assert gs[64].counters.tolist() == [4, 4]  # device dropout step / Adam step == host counters
        want = [rng.stream_key(m.seed, l, generic_train.TRAIN_PASS_BASE + 3) for l in range(len(spec.blocks))]
        assert [k & 0xFFFFFFFF for k in gs[64].keys.tolist()] == want  # the keys step 4 ran with
    return losses, m.store.flat.clone(), m.store.stats.clone(), (m.optimizer.iterations, m._train_step_counter)


@pytest.mark.parametrize("name", ["pooled", "single30"])
def test_graphed_generic_step_matches_eager(name, monkeypatch, deterministic):
    """The HIP-graph replay of the generic step (dropout keys derived on the device from the step
    counter, Adam step from the iteration counter) IS the eager step: in deterministic mode (every
    cross-workgroup sum -- BN moment / backward-sum / bias slots, split-K wgrad partials, head records --
    added in a fixed order) two eager runs and the graph replay give bitwise-identical losses, weights
    and BN statistics after 4 steps.  Atomic mode: only step 1 is compared (identical weights, masks
    and inputs); later steps inherit the fp32 atomics' summation order, which Adam's per-coordinate
    normalisation amplifies (the round-3 driver failure: step-3 |dloss| 0.20)."""
    from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import generic_train, train_ops

    spec = SPECS[name]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(256, spec.input_length, spec.input_channels, generator=g).cuda()
    y = (torch.rand(256, generator=g) < 0.4).float().cuda()
    le, we, se, ce = _generic_steps(monkeypatch, spec, "0", x, y)
    le2, we2, se2, _ = _generic_steps(monkeypatch, spec, "0", x, y)
    lg, wg, sg, cg = _generic_steps(monkeypatch, spec, "1", x, y)
    assert ce == cg == (4, 4)
    assert le2 == le and torch.equal(we2, we) and torch.equal(se2, se)  # reproducible
    assert lg == le, (lg, le)
    assert torch.equal(wg, we) and torch.equal(sg, se)
    train_ops.set_deterministic(False)
    la, _, _, _ = _generic_steps(monkeypatch, spec, "0", x, y)
    lb, _, _, _ = _generic_steps(monkeypatch, spec, "1", x, y)
    assert abs(lb[0] - la[0]) < 1e-4 * abs(la[0])
    assert isinstance(generic_train.GraphedGenericStep, type)
