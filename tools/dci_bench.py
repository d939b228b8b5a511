"""Time the device DCI (metrics.dci_score, csrc/gbt.hip) at the reference's sizes (eval_func: 10 000
training and 5 000 test rows, 100 stages) on synthetic (N, 20) fp32 code tables of the three named
grids, resident on the device.

    python tools/dci_bench.py [--grids shapes3d,mpi3d,cars3d] [--stages 100] [--out dci_bench.json]

Per grid: the whole public call (host sampling, upload, gather, sort, K classifiers, read-back), and
per factor the classifier alone (ops.gbt_fit between two synchronises, tables on the device), with
its class count, launches (3 + 17 per stage) and trees per stage.  The table is factors / sizes plus noise in the
first K columns and noise in the others -- for shapes3d the table tools/gen_golden_dci.py --time gives
the reference's compute_dci on the CPU, which is the comparison.  One warm call of the smallest
factor first; every figure is one timed run (a classifier takes from tenths of a second to seconds).
Prints one JSON line.  There is no pass/fail threshold.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from encdiff_amd import metrics, ops  # noqa: E402

NUM_TRAIN, NUM_TEST, DIMS = 10000, 5000, 20


def table(grid):
    k = grid.num_factors
    f = np.stack(np.unravel_index(np.arange(grid.size), grid.factor_sizes), 1).astype(np.float32)
    rs = np.random.RandomState(0)
    codes = np.concatenate([f / np.array(grid.factor_sizes, np.float32),
                            rs.randn(grid.size, DIMS - k).astype(np.float32)], 1)
    codes[:, :k] += 0.1 * rs.randn(grid.size, k).astype(np.float32)
    return torch.from_numpy(codes).cuda()


def bench_grid(name, stages):
    grid = metrics.FactorGrid.named(name)
    codes = table(grid)
    dev, D = codes.device, codes.shape[1]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    idx_tr, f_tr, idx_te, f_te = metrics.sample_dci(grid, np.random.RandomState(0), NUM_TRAIN, NUM_TEST)
    x_tr = torch.empty(NUM_TRAIN, D, device=dev)
    x_te = torch.empty(NUM_TEST, D, device=dev)
    ops.gbt_gather(codes, up(idx_tr), x_tr)
    ops.gbt_gather(codes, up(idx_te), x_te)
    xs, order = torch.sort(x_tr.t().contiguous(), dim=1, stable=True)
    order = order.to(torch.int32)
    pred_tr = torch.empty(NUM_TRAIN, device=dev, dtype=torch.int32)
    pred_te = torch.empty(NUM_TEST, device=dev, dtype=torch.int32)
    correct = torch.empty(2, device=dev, dtype=torch.int32)
    imp = torch.empty(D, device=dev, dtype=torch.float64)
    factors = []
    order_k = sorted(range(grid.num_factors), key=lambda k: grid.factor_sizes[k])
    for n, k in enumerate([order_k[0]] + list(range(grid.num_factors))):  # the first pass is the warm-up
        c, y_tr, y_te = metrics.dci_labels(f_tr[k], f_te[k])
        t = 1 if c == 2 else c
        ws = torch.empty(ops.gbt_workspace_bytes(NUM_TRAIN, NUM_TEST, D, c), device=dev, dtype=torch.uint8)
        raw_tr = torch.empty(NUM_TRAIN, t, device=dev, dtype=torch.float64)
        raw_te = torch.empty(NUM_TEST, t, device=dev, dtype=torch.float64)
        args = (x_tr, xs, order, up(y_tr), x_te, up(y_te), c, up(metrics.dci_init_raw(y_tr, c)), ws, raw_tr, raw_te,
                pred_tr, pred_te, correct, imp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.gbt_fit(*args, n_estimators=stages)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if n:
            acc = correct.cpu().numpy() / np.array([NUM_TRAIN, NUM_TEST])
            factors.append({"factor": k, "classes": c, "trees_per_stage": t, "launches": 3 + 17 * stages,
                            "enqueue_s": t1 - t0, "total_s": t2 - t0, "acc_train": float(acc[0]),
                            "acc_test": float(acc[1])})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = metrics.dci_score(codes, grid, n_estimators=stages)
    call = time.perf_counter() - t0
    scores.pop("importance_matrix")
    return {"table": list(codes.shape), "factor_sizes": grid.factor_sizes, "factors": factors,
            "classifiers_s": sum(f["total_s"] for f in factors), "dci_score_call_s": call, "scores": scores}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="shapes3d,mpi3d,cars3d")
    ap.add_argument("--stages", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dci_bench needs a HIP device"
    res = {"device": torch.cuda.get_device_name(0), "num_train": NUM_TRAIN, "num_test": NUM_TEST, "stages": a.stages}
    for name in a.grids.split(","):
        res[name] = bench_grid(name, a.stages)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
