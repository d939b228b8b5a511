#!/usr/bin/env python3
"""Warm time of one first-stage decode: the HIP executor (graph replayed) against the torch path of
the same module on the same weights.

    python tools/vq_decode_bench.py --batch 4 --out profiles/vq_decode_bench.jsonl

One batch size per process (appends one JSON line to --out); the recipe in tools/README.md runs
B = 4, 8, 160 (log_images' diffusion rows, samples and swap batch), each under its own timeout.
Both arms decode the same latents (a jittered-lattice codebook, so the quantizer has work to do)
with a disentangled representation.  After warming both arms (the HIP arm until its graph
replays), the arms alternate: each repetition times `--inner` back-to-back decodes per arm with
device events; the figure is the median over the repetitions of the per-decode time.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--config", default="shapes3d")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-quantize", action="store_true", help="the force_not_quantize path")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vq_decode_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vq_decode_bench: no HIP device (a timing needs the GPU)")
    import encdiff_amd  # noqa: F401
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config

    torch.manual_seed(0)
    fs = instantiate_from_config(model_config(a.config)["params"]["first_stage_config"]).cuda().eval()
    n_e, e_dim = fs.quantize.n_e, fs.quantize.e_dim
    H = fs.decoder.z_shape[2]
    g = torch.Generator().manual_seed(1)
    side = max(2, round(n_e ** (1.0 / e_dim)))
    E = (torch.randint(0, side, (n_e, e_dim), generator=g).float() - (side - 1) / 2) * 0.3
    E = E + (torch.rand(n_e, e_dim, generator=g) - 0.5) * 0.03
    with torch.no_grad():
        fs.quantize.embedding.weight.copy_(E.cuda())
    z = (E[torch.randint(0, n_e, (a.batch * H * H,), generator=g)] + torch.randn(a.batch * H * H, e_dim, generator=g) * 0.03)
    z = z.view(a.batch, H, H, e_dim).permute(0, 3, 1, 2).contiguous().cuda()
    s = torch.randn(a.batch, fs.disentangled_dim, generator=g).cuda() if fs.use_disentangled_concat else None
    kw = dict(force_not_quantize=a.no_quantize, disentangled_repr=s)

    fs.enable_hip(decoder=True)
    hip = fs._hip_decoder

    def run_hip():
        return fs.decode(z, **kw)

    def run_torch():
        fs._hip_decoder = None
        try:
            return fs.decode(z, **kw)
        finally:
            fs._hip_decoder = hip

    with torch.no_grad():
        for _ in range(5):  # eager, capture, replays; MIOpen's algorithm search
            out_h, out_t = run_hip(), run_torch()
        assert hip._graphs, "the HIP arm is not replaying a graph"
        err = ((out_h - out_t).norm() / out_t.norm()).item()
        times = {"hip": [], "torch": []}
        for _ in range(a.reps):
            for name, fn in (("hip", run_hip), ("torch", run_torch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.inner)
    res = {"tool": "vq_decode_bench", "config": a.config, "batch": a.batch, "quantize": not a.no_quantize,
           "latent": [e_dim, H, H], "reps": a.reps, "inner": a.inner, "rel_l2_hip_vs_torch": err}
    for name, t in times.items():
        t = sorted(t)
        res[f"{name}_ms_median"] = statistics.median(t)
        res[f"{name}_ms_min"], res[f"{name}_ms_max"] = t[0], t[-1]
    res["speedup_torch_over_hip"] = res["torch_ms_median"] / res["hip_ms_median"]
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
