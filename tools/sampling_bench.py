#!/usr/bin/env python3
"""Wall time of the sampling loops behind log_images beyond plain DDIM.

    python tools/sampling_bench.py --what masked --out profiles/sampling_bench.jsonl

One workload per process (appends one JSON line to --out), each under its own timeout in the
recipe of tools/README.md:

    masked       DDIM with mask + x0 (the centre square of log_images), B = 8, S = 200, eta = 1: steps/s
    quantised    DDIM with quantize_x0, B = 8, S = 200, eta = 1: steps/s
    progressive  progressive_denoising at N = 8, T = 1000: seconds
    log_images   log_images(N = 8) with log_images_full: seconds
    inversion    DDIM inversion (DDIMSamplerAttn.ddim_loop), B = 8, S = 200: steps/s of three arms timed
                 in turn in the same process -- the captured inversion, plain DDIM sampling at eta = 0
                 (the comparison: the same UNet plus one small launch per step) and the eager inversion
                 loop (use_graph=False)

It only calls the public API, so it also runs on a commit from before the captured masked /
quantised paths (where these loops are the eager Python loop); what a commit does not have is
reported as "n/a".  After `--warm` untimed calls (graph captures, MIOpen searches) each of `--reps`
calls is timed host-side around a device synchronize: the loops are host-driven, so the wall time
of a call is the figure.  Reported: every repeat, the median, min and max.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def inversion_arms(ldm, steps, B, shape, cond, x0):
    """{arm: callable} of the inversion workload (None on a commit without DDIMSamplerAttn)."""
    from encdiff_amd.ldm.models.diffusion import ddim as D
    if not hasattr(D, "DDIMSamplerAttn"):
        return None
    inv, plain = ldm.ddim_attn_sampler(), ldm.ddim_sampler()
    eager = D.DDIMSamplerAttn(ldm, use_graph=False)
    return {"inversion": lambda: inv.ddim_loop(x0, cond, steps),
            "ddim_eta0": lambda: plain.sample(steps, B, shape, cond, eta=0.0, verbose=False, x_T=x0),
            "inversion_eager": lambda: eager.ddim_loop(x0, cond, steps)}


def time_arms(arms, a, res):
    """Every round runs each arm once, in turn; the first --warm rounds are not timed."""
    times = {k: [] for k in arms}
    with torch.no_grad():
        for i in range(a.warm + a.reps):
            for k, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= a.warm:
                    times[k].append(time.perf_counter() - t0)
    for k, t in times.items():
        rate = [a.steps / v for v in t]
        res[k] = {"seconds": t, "steps_per_s": rate, "steps_per_s_median": statistics.median(rate),
                  "steps_per_s_min": min(rate), "steps_per_s_max": max(rate)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=["masked", "quantised", "progressive", "log_images", "inversion"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--timesteps", type=int, default=1000, help="progressive: start_T")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampling_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sampling_bench: no HIP device (a timing needs the GPU)")
    import encdiff_amd  # noqa: F401
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config

    torch.manual_seed(0)
    ldm = instantiate_from_config(model_config("shapes3d")).cuda()
    ldm.setup_hip_training()
    B, H = a.batch, ldm.image_size
    g = torch.Generator().manual_seed(1)
    cond = (torch.randn(B, 320, generator=g) * 0.5).cuda()
    x0 = torch.randn(B, ldm.channels, H, H, generator=g).cuda()
    mask = torch.ones(B, 1, H, H, device="cuda")
    mask[:, :, H // 4:3 * H // 4, H // 4:3 * H // 4] = 0.
    img = (torch.rand(B, 64, 64, 3, generator=g) * 2 - 1).cuda()
    shape = (ldm.channels, H, H)
    res = {"tool": "sampling_bench", "what": a.what, "batch": B, "reps": a.reps, "warm": a.warm}

    fn, work = None, None
    if a.what in ("masked", "quantised"):
        sampler = ldm.ddim_sampler()
        kw = dict(mask=mask, x0=x0) if a.what == "masked" else dict(quantize_x0=True)
        fn = lambda: sampler.sample(a.steps, B, shape, cond, eta=1.0, verbose=False, **kw)  # noqa: E731
        work = a.steps
        res["steps"] = a.steps
    elif a.what == "progressive":
        if hasattr(ldm, "progressive_denoising"):
            fn = lambda: ldm.progressive_denoising(cond, shape=shape, batch_size=B, verbose=False,  # noqa: E731
                                                   start_T=a.timesteps)
        res["timesteps"] = a.timesteps
    elif a.what == "inversion":
        res["steps"] = a.steps
        arms = inversion_arms(ldm, a.steps, B, shape, cond, x0)
        if arms is not None:
            time_arms(arms, a, res)
            res["graphs"] = sorted({k[0] for k in ldm.ddim_attn_sampler()._graphs} |
                                   {k[0] for k in ldm.ddim_sampler()._graphs})
    else:
        if hasattr(type(ldm), "log_images_full"):
            ldm.log_images_full = True
            fn = lambda: ldm.log_images({"image": img}, N=B, ddim_steps=a.steps)  # noqa: E731
        res["steps"] = a.steps

    if a.what == "inversion" and "inversion" in res:
        pass  # the three arms are in res
    elif fn is None:
        res["seconds_median"] = "n/a"
    else:
        times = []
        with torch.no_grad():
            for i in range(a.warm + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= a.warm:
                    times.append(time.perf_counter() - t0)
        res["seconds"] = times
        res["seconds_median"] = statistics.median(times)
        res["seconds_min"], res["seconds_max"] = min(times), max(times)
        if work:
            res["steps_per_s"] = [work / t for t in times]
            res["steps_per_s_median"] = work / res["seconds_median"]
        if a.what in ("masked", "quantised"):
            res["graphs"] = sorted({k[0] for k in getattr(ldm.ddim_sampler(), "_graphs", {})})
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
