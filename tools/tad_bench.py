"""Time the device TAD (encdiff_amd.metrics.tad_aurocs, csrc/tad.hip) at CelebA's sizes with this
project's 40 x 16 = 640 token columns and 40 attributes: the test split (N = 19962) and the whole
set (N = 202599), on synthetic tokens resident on the device.

    python tools/tad_bench.py [--reps 20] [--out tad_bench.json]

Each shape runs in a child process of its own under a time limit (a fault or hang in one ends the
tool: nothing more is started); at most 16 CPU threads.  Per shape, all warm (one untimed call first):
  call      the whole public tad_aurocs: label packing (torch), the four ops, read-back of the joint
            table; host clock around the call, which ends in that device-to-host read;
  per op    device events around `inner` back-to-back launches of one op, divided by `inner`;
            tad_counts and tad_label_joint include their zeroing kernel;
  counts    bytes the counting op must move (z once, the label words, the thresholds, the counts)
            over its time, against the 8 TB/s of HBM (MI355X).
Prints one JSON line.  There is no pass/fail threshold.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(19962, 640, 40), (202599, 640, 40)]
HBM_BYTES_PER_S = 8e12
STEP_LIMIT_S = 240


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": len(ts)}


def run_shape(n, L, A, reps, inner):
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, REPO)
    from encdiff_amd import metrics, ops
    assert torch.cuda.is_available(), "tad_bench needs a HIP device"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    targ = (torch.rand(n, A, device=dev, generator=g) < torch.linspace(0.05, 0.8, A, device=dev)).to(torch.uint8)
    z = torch.randn(n, L, device=dev, generator=g)
    z[:, :A] += 2.0 * targ.to(torch.float32)  # some columns carry an attribute
    res = {"n": n, "L": L, "A": A}

    out = {}

    def call():
        out.update(metrics.tad_aurocs(z, targ))

    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    res["tad_aurocs_call"] = stats(ts)

    packed = metrics.pack_attributes(targ)
    t = metrics.tad_thresholds().to(dev)
    f32 = dict(device=dev, dtype=torch.float32)
    ma, mi, thr = torch.empty(L, **f32), torch.empty(L, **f32), torch.empty(L, 11, **f32)
    counts = torch.empty(ops.tad_counts_shape(L, A), device=dev, dtype=torch.int32)
    joint = torch.empty(A, A, device=dev, dtype=torch.int32)
    au = torch.empty(A, L, **f32)
    steps = (("tad_range", lambda: ops.tad_range(z, t, ma, mi, thr)),
             ("tad_counts", lambda: ops.tad_counts(z, packed, A, thr, counts)),
             ("tad_label_joint", lambda: ops.tad_label_joint(packed, A, joint)),
             ("tad_auroc", lambda: ops.tad_auroc(counts, joint, ma, mi, n, au)))
    for name, fn in steps:
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / inner)
        res[name] = stats(ts)
    assert torch.equal(au.view(torch.int32), out["aurocs"].view(torch.int32))
    nbytes = n * L * 4 + n * 8 + L * 11 * 4 + counts.numel() * 4
    rate = nbytes / (1e-3 * res["tad_counts"]["median_ms"])
    res["tad_counts_bytes"] = nbytes
    res["tad_counts_bytes_per_s"] = rate
    res["tad_counts_share_of_hbm"] = rate / HBM_BYTES_PER_S
    res["inner"] = inner
    res["device"] = torch.cuda.get_device_name(0)
    res["max_auroc"] = float(np.nanmax(au.cpu().numpy()))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="N,L,A: run this shape in this process")
    a = ap.parse_args()
    if a.shape:
        return run_shape(*(int(v) for v in a.shape.split(",")), a.reps, a.inner)
    shapes = []
    for n, L, A in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", f"{n},{L},{A}", "--reps", str(a.reps),
               "--inner", str(a.inner)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"shape {(n, L, A)} ended with status {r.returncode}: nothing more is started")
        shapes.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps({"hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": shapes})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
