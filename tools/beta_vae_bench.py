"""Time the beta-VAE score and the token PCA on the device at eval_func's sizes (main_val.py:38-65):
beta_vae_score (10 000 training and 5 000 evaluation points of 64 row pairs, D = 20) on synthetic
code tables of the Shapes3D and MPI3D grids, and token_pca on a (480 000, 20, 16) fp32 token array.

    python tools/beta_vae_bench.py [--reps 10] [--out beta_vae_bench.json]

All figures are warm (one untimed call first), host clock around calls that end in a read-back or
between two synchronises, median with min and max over --reps runs:
  call      the whole public call: host index sampling, uploads, the kernels, read-back;
  features, fit, predict
            the kernels alone on tables already on the device; the fit's time is also given per loss
            evaluation (its n_fev comes back with it);
  moments, project
            the two streaming kernels of token_pca alone, with the bytes of the token array over the
            time as achieved bandwidth (both read the array once; the chip streams about 6.3 TB/s).
The code table is the one tools/gen_golden_beta_vae.py --time gives the reference on the CPU.
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from encdiff_amd import metrics, ops  # noqa: E402

STREAM_TBS = 6.3  # measured float4 copy rate of the chip


def table(grid):
    f = np.stack(np.unravel_index(np.arange(grid.size), grid.factor_sizes), 1).astype(np.float32)
    rs = np.random.RandomState(0)
    k = grid.num_factors
    codes = np.concatenate([f / np.array(grid.factor_sizes, np.float32), rs.randn(grid.size, 20 - k).astype(np.float32)], 1)
    codes[:, :k] += 0.1 * rs.randn(grid.size, k).astype(np.float32)
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


def bench_score(name, reps):
    grid = metrics.FactorGrid.named(name)
    codes = table(grid)
    dev, D, K = codes.device, codes.shape[1], grid.num_factors
    res = {"table": list(codes.shape), "factor_sizes": grid.factor_sizes}
    score = {}

    def call():
        score.update(metrics.beta_vae_score(codes, grid, return_fit=True))

    res["call"] = timed(call, reps)
    res["scores"] = {k: score[k] for k in ("train_accuracy", "eval_accuracy", "n_iter", "n_fev", "status", "loss")}
    rs = np.random.RandomState(0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    idx1, idx2, labels = (up(x) for x in metrics.sample_beta_vae(grid, rs, 64, 10000))
    f64 = dict(device=dev, dtype=torch.float64)
    x = torch.empty(10000, D, **f64)
    coef, intercept, loss = torch.empty(K, D, **f64), torch.empty(K, **f64), torch.empty(1, **f64)
    info = torch.empty(4, device=dev, dtype=torch.int32)
    correct = torch.empty(1, device=dev, dtype=torch.int32)
    ws = torch.empty(ops.logreg_workspace_bytes(10000, D, K), device=dev, dtype=torch.uint8)
    res["features"] = timed(lambda: ops.beta_features(codes, idx1, idx2, x), reps)
    res["fit"] = timed(lambda: ops.logreg_fit(x, labels, K, ws, coef, intercept, info, loss), reps)
    n_fev = int(info[1].item())
    res["fit"]["n_fev"] = n_fev
    res["fit"]["per_evaluation_us"] = 1e3 * res["fit"]["median_ms"] / n_fev
    res["predict"] = timed(lambda: ops.logreg_predict(x, labels, coef, intercept, correct), reps)
    return res


def bench_pca(reps, shape=(480000, 20, 16)):
    import logreg_restate as R
    tokens = torch.from_numpy(R.make_tokens(shape)).cuda()
    n, u, d = shape
    dev = tokens.device
    res = {"tokens": list(shape), "bytes": tokens.numel() * 4}
    out = {}

    def call():
        out["r"] = metrics.token_pca(tokens)

    res["call"] = timed(call, reps)
    mean = torch.empty(u, d, device=dev, dtype=torch.float64)
    cov = torch.empty(u, d, d, device=dev, dtype=torch.float64)
    ws = torch.empty(ops.token_workspace_bytes(n, u, d), device=dev, dtype=torch.uint8)
    comps = torch.from_numpy(out["r"][1]).to(dev)
    codes = torch.empty(n, u, device=dev)
    res["moments"] = timed(lambda: ops.token_moments(tokens, ws, mean, cov), reps)
    res["project"] = timed(lambda: ops.token_project(tokens, mean, comps, codes), reps)
    for k in ("moments", "project"):
        tbs = res["bytes"] / (1e-3 * res[k]["median_ms"]) / 1e12
        res[k]["achieved_TBs"] = tbs
        res[k]["of_streaming_rate"] = tbs / STREAM_TBS
    res["explained_variance_first_units"] = [float(v) for v in out["r"][3][:3]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "beta_vae_bench needs a HIP device"
    res = {"device": torch.cuda.get_device_name(0), "num_train": 10000, "num_eval": 5000, "batch": 64}
    for name in ("shapes3d", "mpi3d"):
        res[name] = bench_score(name, a.reps)
    res["token_pca"] = bench_pca(a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
