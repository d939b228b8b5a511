"""Time the device metrics at the reference's sizes (eval_func, main_val.py:74-94): factor_vae_score
(batch 64, 10000 + 5000 votes, 10000 rows of variance estimate) and mig_score (10000 rows, 20 bins) on
a synthetic Shapes3D-sized (480000, 20) fp32 code table resident on the device.

    python tools/metrics_bench.py [--reps 20] [--out metrics_bench.json]

Two figures per metric, both warm (one untimed call first), host clock around calls that end in a
device-to-host read of the result:
  call     the whole public call: host index sampling (numpy RandomState, reference order), upload of
           the index tables, the kernels, read-back of votes / score;
  device   the kernels alone on index tables already on the device, between two synchronises.
The table is factors / sizes plus noise in the first six columns and noise in the other fourteen --
the table tools/gen_golden_metrics.py --time gives the reference's functions on the CPU.
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


def table(grid):
    f = np.stack(np.unravel_index(np.arange(grid.size), grid.factor_sizes), 1).astype(np.float32)
    rs = np.random.RandomState(0)
    codes = np.concatenate([f / np.array(grid.factor_sizes, np.float32),
                            rs.randn(grid.size, 14).astype(np.float32)], 1)
    codes[:, :6] += 0.1 * rs.randn(grid.size, 6).astype(np.float32)
    return torch.from_numpy(codes).cuda()


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": len(ts)}


def timed(fn, reps):
    fn()  # warm
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs a HIP device"
    grid = metrics.FactorGrid.named("shapes3d")
    codes = table(grid)
    dev, D, K = codes.device, codes.shape[1], grid.num_factors
    res = {"table": list(codes.shape), "device": torch.cuda.get_device_name(0)}
    scores = {}

    def fv_call():
        scores["factor_VAE"] = metrics.factor_vae_score(codes, grid)

    def mig_call():
        scores["MIG"] = metrics.mig_score(codes, grid)

    res["factor_vae_score_call"] = timed(fv_call, a.reps)
    res["mig_score_call"] = timed(mig_call, a.reps)

    # the kernels alone, tables on the device
    rs = np.random.RandomState(0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    var_idx = up(metrics.sample_variance_indices(grid, rs, 10000))
    tr = [up(x) for x in metrics.sample_votes(grid, rs, 64, 10000)]
    ev = [up(x) for x in metrics.sample_votes(grid, rs, 64, 5000)]
    gvar = torch.empty(D, device=dev, dtype=torch.float64)
    vt, ve = (torch.empty(K, D, device=dev, dtype=torch.int32) for _ in range(2))

    def fv_dev():
        ops.gather_colvar(codes, var_idx, gvar)
        ops.fvae_votes(codes, tr[0], tr[1], K, gvar, 0.05, vt)
        ops.fvae_votes(codes, ev[0], ev[1], K, gvar, 0.05, ve)

    midx, mfac = (up(x) for x in metrics.sample_mig(grid, np.random.RandomState(0), 10000))
    edges = torch.empty(D, 20, device=dev)
    counts = torch.empty(ops.mig_counts_shape(D, grid.factor_sizes), device=dev, dtype=torch.int32)
    mi = torch.empty(D, K, device=dev, dtype=torch.float64)
    h = torch.empty(K, device=dev, dtype=torch.float64)
    score = torch.empty(1, device=dev, dtype=torch.float64)

    def mig_dev():
        ops.mig_hist(codes, midx, mfac, grid.factor_sizes, edges, counts)
        ops.mig_finalize(counts, grid.factor_sizes, 10000, mi, h, score)

    def many(fn, n=50):  # 50 back-to-back runs per timed window: the kernels take well under a ms
        return lambda: [fn() for _ in range(n)]

    for name, fn in (("factor_vae_device", fv_dev), ("mig_device", mig_dev)):
        s = timed(many(fn), a.reps)
        res[name] = {k: (v / 50 if k.endswith("_ms") else v) for k, v in s.items()}
    assert float(score.item()) == scores["MIG"]["discrete_mig"]
    res["scores"] = scores
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
