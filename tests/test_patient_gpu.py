"""GPU: the patient kernels (``csrc/uq_patient.hip``) against the integer emulation of ``ops/patient.py``,
bit for bit, and the public API on CUDA predictions against the float64 golden."""
import numpy as np
import pytest
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import patient as P
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import uq as uq_ops
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import metrics as M
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import patient_level as PL

from .patient_fixtures import assert_labels_unambiguous, check_cohort, check_table, cohort

pytestmark = pytest.mark.gpu

SHARDS = ((0, 1000), (1000, 1001), (1001, 3001))
B = 16
N, N_PAT = 3001, 37


def _grouped_codes(n, n_pat, seed):
    """Sorted codes with uneven runs: code 0 has one window, code 1 more than 256 (a run over several of a
    wave's ranges), code 2 has none, the other boundaries fall anywhere."""
    rs = np.random.RandomState(seed)
    if n_pat == 1:
        return np.zeros(n, dtype=np.int32)
    rest = np.sort(rs.choice(np.arange(3, n_pat), n - 1 - 300, replace=True))
    code = np.concatenate([[0], np.full(300, 1), rest]).astype(np.int32)
    starts = np.flatnonzero(np.diff(code)) + 1
    assert len(code) == n and np.sum(code == 2) == 0 and np.mean(starts % 64 != 0) > 0.9
    return code


def _inputs(t_count, n, n_pat, seed=1, shuffle=False, sparse=False):
    """probs whose first windows carry p = 0, 1, 0.5 and NaN, labels, codes; m is made on the device."""
    rs = np.random.RandomState(seed)
    p = rs.rand(t_count, n).astype(np.float32)
    p[:, 0], p[:, 1], p[:, 2] = 0.0, 1.0, 0.5
    p[0, 3] = np.nan
    y = (rs.rand(n) > 0.7).astype(np.int32)
    code = rs.randint(0, n_pat, size=n).astype(np.int32) if sparse else _grouped_codes(n, n_pat, seed)
    if shuffle:
        perm = rs.permutation(n)
        p, y, code = np.ascontiguousarray(p[:, perm]), y[perm], code[perm]
    return torch.from_numpy(p), torch.from_numpy(y), torch.from_numpy(code)


def _both(p, y, code, n_pat):
    """(device outputs, emulation outputs) from the same device-made per-window rows."""
    pc = p.cuda()
    m = uq_ops.metrics(pc)
    got = P.reduce(pc, m, y.cuda(), code.cuda(), n_pat)
    ref = P.reduce_eager(p, m.cpu(), y, code, n_pat)
    return got, ref


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("t_count", [1, 3, 50, 70])
def test_patient_reduce_matches_eager(t_count, shuffle):
    _ext.require()
    p, y, code = _inputs(t_count, N, N_PAT, shuffle=shuffle)
    got, ref = _both(p, y, code, N_PAT)
    assert got[0].dtype == torch.int32 and tuple(got[0].shape) == (t_count, N_PAT)
    assert got[1].dtype == torch.int64 and tuple(got[1].shape) == (N_PAT, P.N_REC)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
    assert int(got[1][:, 0].sum()) == N and int(got[1][2].abs().sum()) == 0 and int(got[0][:, 2].sum()) == 0
    assert int(got[1][0, 0]) == 1 and int(got[1][1, 0]) == 300
    again = P.reduce(p.cuda(), uq_ops.metrics(p.cuda()), y.cuda(), code.cuda(), N_PAT)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_patient_reduce_single_patient_and_many_patients():
    _ext.require()
    p, y, code = _inputs(50, N, 1)
    got, ref = _both(p, y, code, 1)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
    assert got[0][:, 0].cpu().tolist() == (p > 0.5).sum(1).tolist()
    # T P = 250,000 counters (no workgroup table could hold them), most patients with one or two windows
    p, y, code = _inputs(50, 6000, 5000, sparse=True)
    got, ref = _both(p, y, code, 5000)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
    # codes outside [0, P) are skipped
    bad = code.clone()
    bad[::7] = -1
    bad[3::7] = 5000
    got, ref = _both(p, y, bad, 5000)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
    assert int(got[1][:, 0].sum()) == int(((bad >= 0) & (bad < 5000)).sum())


@pytest.mark.parametrize("shuffle", [False, True])
def test_patient_reduce_shards_add(shuffle):
    _ext.require()
    p, y, code = _inputs(50, N, N_PAT, shuffle=shuffle)
    pc, yc, cc = p.cuda(), y.cuda(), code.cuda()
    m = uq_ops.metrics(pc)
    whole = P.reduce(pc, m, yc, cc, N_PAT)
    pass_pos, rec = torch.zeros_like(whole[0]), torch.zeros_like(whole[1])
    for lo, hi in SHARDS:
        a, b = P.reduce(pc[:, lo:hi].contiguous(), m[:, lo:hi].contiguous(), yc[lo:hi], cc[lo:hi], N_PAT)
        pass_pos += a
        rec += b
    assert torch.equal(pass_pos, whole[0]) and torch.equal(rec, whole[1])


@pytest.fixture(scope="module")
def records():
    """(P, 25) records with every class, both signs of the error and large fixed-point sums."""
    def get(n_pat):
        rs = np.random.RandomState(n_pat)
        prec = rs.randint(0, 1 << 40, size=(n_pat, P.N_PREC)).astype(np.int64)
        prec[:, P.TRUE_CLASS], prec[:, P.PRED_CLASS] = rs.randint(0, 4, n_pat), rs.randint(0, 4, n_pat)
        prec[:, P.COL["err_q"]] -= 1 << 39
        return torch.from_numpy(prec)

    return get


@pytest.mark.parametrize("parity", [True, False])
@pytest.mark.parametrize("n_pat", [1, 37, 700])
def test_patient_bootstrap_matches_eager(records, n_pat, parity):
    _ext.require()
    prec = records(n_pat)
    idx = torch.from_numpy(M.parity_bootstrap_indices(n_pat, B, 7).astype(np.int32)) if parity else None
    got = P.bootstrap_sums(prec.cuda(), B, idx=None if idx is None else idx.cuda(), seed=7)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, P.N_SUMS)
    assert torch.equal(got.cpu(), P.bootstrap_sums_eager(prec, idx, 7, B))
    assert torch.equal(got[:, P.N_PREC:].sum(1).cpu(), torch.full((B,), n_pat))
    assert torch.equal(P.bootstrap_sums(prec.cuda(), B, idx=None if idx is None else idx.cuda(), seed=7), got)
    if not parity:  # the keying of ops.uq.bootstrap with n = P
        draws = uq_ops._hash_idx(n_pat, B, 7, "cpu")
        assert torch.equal(got[:, :P.N_PREC].cpu(), torch.stack([prec[d].sum(0) for d in draws]))


def test_patient_bootstrap_rejects_overflow(records):
    _ext.require()
    big = records(37).clone()
    big[5, 5] = 1 << 61
    with pytest.raises(RuntimeError):
        torch.ops.apneauq.patient_bootstrap(big.cuda(), None, 0, 1)
    with pytest.raises(RuntimeError):
        torch.ops.apneauq.patient_bootstrap(records(37)[:, :24].contiguous().cuda(), None, 0, 1)


def test_public_api_on_cuda_predictions():
    _ext.require()
    probs, y, ids = cohort(2)
    assert_labels_unambiguous(probs)
    pc = torch.from_numpy(probs).cuda()
    ref = PL.golden_patient_table(probs, y, ids)
    got = PL.patient_table(pc, y, ids)
    check_table(got, ref)
    point = PL.golden_cohort(ref, probs, y, ids)
    for parity in (True, False):
        res = PL.evaluate_patient_level(pc, y, ids, "gpu", n_bootstrap=B, random_state=11, parity=parity,
                                        make_plots=False)
        check_cohort(res, point, ref)
        idx = M.parity_bootstrap_indices(40, B, 11) if parity else uq_ops._hash_idx(40, B, 11, "cpu").numpy()
        rep = PL.golden_cluster_replicates(ref, probs, y, ids, idx)
        lower = {k: float(np.nanpercentile([r[k] for r in rep], 2.5)) for k in PL.COHORT_KEYS}
        upper = {k: float(np.nanpercentile([r[k] for r in rep], 97.5)) for k in PL.COHORT_KEYS}
        check_cohort(res, lower, ref, "_ci_lower")
        check_cohort(res, upper, ref, "_ci_upper")
        for k in PL.COHORT_KEYS:
            assert res[f"{k}_ci_lower"] <= res[k] <= res[f"{k}_ci_upper"], (k, parity)
