"""Speed of the ensemble-composition analysis: the ``member_pairs`` and ``member_mix`` kernels against the torch
float64 formulation of the same quantities on the same GPU, the whole ``select_members`` and
``evaluate_members`` calls, and the golden NumPy greedy loop.

``python -m bench.members_micro [--out profiles/members_micro.json]`` measures, at T = 50 and T = 20 members and
16,384, 131,072 and 1,048,576 windows, with the predictions already on the GPU:

* ``kernel_ms`` (HIP events around the op, median of ``kernel_runs`` after a warm-up; the op includes the zero
  fill of its output, for ``member_pairs`` the mirror of the triangle and for ``member_mix`` the host check and
  the upload of the counts): ``member_pairs`` at the launcher's grid and at ``--grids``; ``member_mix`` with T rows
  "member 0 plus member m" (a greedy step) and with 64 rows of k = T / 2 random members, with and without five
  folds.
  ``pair_products_per_s`` is T (T + 1) / 2 x n products per launch over the time, ``mix_bytes_per_s`` the bytes
  the launch has to read once (probabilities, labels, fold codes) over the time: both computed from the shapes.
* ``torch_ms`` (the same clock): the binary and residual Grams as three float64 matmuls; and
  ``(counts @ probs) / k``, the two losses, the three label counts and their sums per fold as a float64
  matmul with the one-hot folds.  These are not quantised and not bit-reproducible; they are what a user
  would write.
* ``wall_ms`` (host clock around work that ends in a device synchronise, median of ``runs`` after a warm-up
  call): ``select_members`` over the whole path k = 1..T without folds and with five patient folds, and
  ``evaluate_members(..., make_plots=False)`` without files.
* ``golden_select``: the NumPy greedy loop on the same machine's CPU for ``golden_steps`` steps (the record
  says how many; a whole path is T steps).

A measurement path that finds no GPU fails.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import _ext
from uncertaintyquantification_sleepapnea_1dcnn_amd.ops import members as MB
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq import members as MM
from uncertaintyquantification_sleepapnea_1dcnn_amd.uq.recalibration import assign_folds

from .calib_micro import _events, _wall
from .convergence_micro import synthetic

SEED = 2025
FOLDS = 5


def torch_pairs(p, y):
    """The three Grams in float64: both correct and y = 0, both correct and y = 1, residuals."""
    ok = torch.isfinite(p).all(0)
    pv, y1 = p[:, ok], y[ok] != 0
    r = pv.double() - y1.double()
    c = (pv > 0.5) == y1
    c0, c1 = (c & ~y1).double(), (c & y1).double()
    return c0 @ c0.T, c1 @ c1.T, r @ r.T


def torch_mix(p, y, counts, onehot):
    """Per fold and row: n, n_y1, the NLL and Brier sums and the three label counts, in float64."""
    ok = torch.isfinite(p).all(0)
    pv, y1, oh = p[:, ok].double(), y[ok] != 0, onehot[:, ok]
    k = counts.sum(1, keepdim=True)
    s = counts @ pv
    m = s / k
    lab = 2.0 * s > k
    nll = -torch.log(torch.where(y1, m, 1.0 - m).clamp(1e-7, 1 - 1e-7))
    brier = (m - y1.double()) ** 2
    cols = [torch.ones_like(m), y1.double().expand_as(m), nll, brier, (lab == y1).double(), (lab & y1).double(), lab.double()]
    return torch.stack([v @ oh.T for v in cols], dim=-1)


def measure(n, t_count, grids, runs, kernel_runs, golden_steps):
    probs, y = synthetic(n, t_count)
    pc, yt = torch.from_numpy(probs).cuda(), torch.from_numpy(y).cuda()
    rs = np.random.RandomState(SEED)
    pid = np.sort(rs.randint(0, max(FOLDS, n // 800), size=n))
    fold = torch.from_numpy(assign_folds(pid, FOLDS, SEED).astype(np.uint8)).cuda()
    ops = _ext.ops()
    out = {"windows": n, "members": t_count}

    # ---- member_pairs ----
    products = t_count * (t_count + 1) // 2 * n
    kp = {"auto": _events(lambda: ops.member_pairs(pc, yt, 0, 0), kernel_runs), "grid": {}}
    for g in grids:
        kp["grid"][str(g)] = _events(lambda: ops.member_pairs(pc, yt, g, 0), kernel_runs)
    kp["pair_products_per_s"] = round(products / (kp["auto"] * 1e-3), 0)
    tp = _events(lambda: torch_pairs(pc, yt), kernel_runs)

    # ---- member_mix ----
    eye = np.eye(t_count, dtype=np.int64)
    step_rows = eye[0][None] + eye                        # T rows: member 0 plus member m
    half = np.zeros((64, t_count), np.int64)
    for q in range(64):
        half[q, rs.permutation(t_count)[:t_count // 2]] = 1
    nbytes = n * (4 * t_count + 4)
    km, tm = {}, {}
    for name, rows in (("greedy_step", step_rows), ("64_rows_half", half)):
        ci = torch.from_numpy(rows).to(torch.int32)   # the op takes the counts as a host tensor
        cd = ci.cuda().double()
        oh1 = torch.ones(1, n, dtype=torch.float64, device="cuda")
        oh5 = torch.nn.functional.one_hot(fold.long(), FOLDS).T.double().contiguous()
        t1 = _events(lambda: ops.member_mix(pc, yt, None, ci, 1, 0), kernel_runs)
        t5 = _events(lambda: ops.member_mix(pc, yt, fold, ci, FOLDS, 0), kernel_runs)
        km[name] = {"rows": int(len(rows)), "no_folds": t1, "five_folds": t5,
                    "mix_bytes_per_s": round(nbytes / (t1 * 1e-3), 0),
                    "mix_bytes_per_s_five_folds": round((nbytes + n) / (t5 * 1e-3), 0)}
        tm[name] = {"no_folds": _events(lambda: torch_mix(pc, yt, cd, oh1), kernel_runs),
                    "five_folds": _events(lambda: torch_mix(pc, yt, cd, oh5), kernel_runs)}
    out["kernel_ms"] = {"member_pairs": kp, "member_mix": km}
    out["torch_ms"] = {"member_pairs": tp, "member_mix": tm}

    # ---- whole calls ----
    out["wall_ms"] = {
        "select_members": _wall(lambda: MM.select_members(pc, y), runs),
        "select_members_five_folds": _wall(lambda: MM.select_members(pc, y, groups=pid, n_folds=FOLDS), runs),
        "evaluate_members": _wall(lambda: MM.evaluate_members(pc, y, "bench", patient_ids=pid, n_folds=FOLDS,
                                                              output_dir=None, make_plots=False), runs)}
    if golden_steps > 0:
        t = time.perf_counter()
        MM.golden_select(probs, y, "nll", golden_steps)
        out["golden_select"] = {"ms": round((time.perf_counter() - t) * 1e3, 1), "steps": golden_steps,
                                "steps_of_a_whole_path": t_count}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16384,131072,1048576")
    ap.add_argument("--members", default="50,20")
    ap.add_argument("--grids", default="8,32,64,256,1024", help="member_pairs grids timed next to the launcher's choice")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kernel_runs", type=int, default=50)
    ap.add_argument("--golden_steps", default="50,3,1", help="greedy steps of the NumPy loop per size (0: skip it)")
    ap.add_argument("--out", default=os.path.join("profiles", "members_micro.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("members_micro: no GPU; nothing is measured without one")
    _ext.require()
    sizes = [int(v) for v in a.sizes.split(",")]
    gs = [int(v) for v in a.golden_steps.split(",")]
    gs += [gs[-1]] * (len(sizes) - len(gs))
    res = {"bench": "members_micro", "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
           "reduction": "64-bit integer atomics, once per workgroup",
           "not_measured": ["other member counts than those listed", "occupancy", "hardware counters",
                            "multi-rank runs"],
           "results": []}
    for t_count in (int(v) for v in a.members.split(",")):
        for n, g in zip(sizes, gs):
            r = measure(n, t_count, [int(v) for v in a.grids.split(",")], a.runs, a.kernel_runs, min(g, t_count))
            res["results"].append(r)
            print(json.dumps(r), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    return res


if __name__ == "__main__":
    main()
