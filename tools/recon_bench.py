"""Time the reconstruction scores (csrc/recon.hip) and the loop they end.

    python tools/recon_bench.py [--reps 20] [--images 128] [--steps 200] [--out profiles/recon_bench.json]

Figures, all warm (untimed calls first), all on the device this runs on:
  kernel    encdiff_ssim_mse alone at 128 images, in the reference layout (128, 64, 64, 3) -- x0 as
            the data gives it, the reconstruction an NCHW tensor permuted by strides -- and in nchw
            (128, 3, 64, 64): 50 launches captured into one graph, device events around a replay,
            divided by 50 (no host time in it), and the same 50 launches eager (host included);
  torch     the same two scores formed with torch's five float32 depthwise F.conv2d calls on
            premapped inputs, eager, device events around 50 calls (what a user had to write before);
            its largest deviation from the kernel is reported next to it;
  loop      LatentDiffusion.reconstruction_metrics on a synthetic pool at S = `steps`, eta = 1,
            batch 64 (a randomly initialised shapes3d model: the time does not depend on the
            weights), host clock around the whole call, which ends in its read-back; and the
            kernel's share of it: batches x the graph-replayed kernel time at the batch shape.
Prints one JSON line.  There is no pass/fail threshold.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from encdiff_amd import metrics, ops  # noqa: E402
from encdiff_amd.graph_loops import capture  # noqa: E402

INNER = 50


def stats(ts, div=1):
    ts = sorted(t / div for t in ts)
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": len(ts)}


def event_ms(fn, reps):
    """Device time of fn() (which only enqueues), per call, between two events."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def torch_scores(a, b, window):
    """SSIM and MSE from five depthwise convolutions in float32, a and b (B, Ch, H, W) in [0, 1]."""
    ch = a.shape[1]
    w = window.expand(ch, 1, 11, 11).contiguous()
    conv = lambda x: F.conv2d(x, w, padding=5, groups=ch)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return ssim.mean(dim=[1, 2, 3]), (a - b).pow(2).mean(dim=[1, 2, 3])


def kernel_figures(x0, x_recon, layout, reps):
    a, b = metrics.reconstruction_views(x0, x_recon, layout)
    n = a.shape[0]
    s, m = torch.empty(n, device="cuda", dtype=torch.float64), torch.empty(n, device="cuda", dtype=torch.float64)

    def many():
        for _ in range(INNER):
            ops.ssim_mse(a, b, 1., 0.5, out_ssim=s, out_mse=m)

    many()
    graph = capture(many)
    res = {"shape": list(a.shape), "strides_a": list(a.stride()), "strides_b": list(b.stride()),
           "kernel_graph": stats(event_ms(graph.replay, reps), INNER),
           "kernel_eager": stats(event_ms(many, reps), INNER)}
    pa, pb = ((a + 1.) / 2.).contiguous(), ((b + 1.) / 2.).contiguous()
    win = metrics.ssim_window().cuda()
    res["torch_conv2d_eager"] = stats(event_ms(lambda: [torch_scores(pa, pb, win) for _ in range(INNER)], reps), INNER)
    ts, tm = torch_scores(pa, pb, win)
    res["torch_minus_kernel"] = {"ssim": float((ts.double() - s).abs().max()), "mse": float((tm.double() - m).abs().max())}
    res["ssim_mean"] = float(s.mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "recon_bench needs a HIP device"
    g = torch.Generator(device="cuda").manual_seed(0)
    n = a.images
    x0 = torch.rand(n, 64, 64, 3, device="cuda", generator=g) * 2 - 1
    x_recon = (x0.permute(0, 3, 1, 2) + 0.1 * torch.randn(n, 3, 64, 64, device="cuda", generator=g)).clamp(-1, 1).contiguous()
    res = {"device": torch.cuda.get_device_name(0), "images": n,
           "reference_layout": kernel_figures(x0, x_recon, "reference", a.reps),
           "nchw": kernel_figures(x0, x_recon, "nchw", a.reps)}

    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    torch.manual_seed(0)
    model = instantiate_from_config(model_config("shapes3d")).cuda()
    pool = torch.randint(0, 256, (n, 64, 64, 3), device="cuda", dtype=torch.uint8, generator=g)
    batch = 64
    call = lambda: model.reconstruction_metrics(pool=pool, ddim_steps=a.steps, eta=1., batch_size=batch)  # noqa: E731
    call()  # captures the sampling graphs
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.loop_reps):
        t0 = time.perf_counter()
        out = call()
        ts.append(1e3 * (time.perf_counter() - t0))
    b = min(batch, n)
    at_batch = kernel_figures(x0[:b], x_recon[:b].contiguous(), "reference", a.reps)["kernel_graph"]["median_ms"]
    batches = -(-n // batch)
    loop = stats(ts)
    res["reconstruction_metrics"] = {"ddim_steps": a.steps, "eta": 1.0, "batch_size": batch, "batches": batches,
                                     "call": loop, "kernel_ms_per_batch": at_batch,
                                     "kernel_share": batches * at_batch / loop["median_ms"],
                                     "ssim": out["ssim"], "mse": out["mse"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
