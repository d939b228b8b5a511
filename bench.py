"""EncDiff training benchmark on MI355X (driver contract: one JSON line on rank 0).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...   (data-parallel, RCCL)

Metric (BASELINE.json): training imgs/sec on Shapes3D 64x64 (VQ-f4, 16x16 latent),
configs[1]: batch 128 per GPU, bf16 HIP path.  A step = one full LatentDiffusion
training step: frozen VQ encode + Encoder4 + q_sample + UNet fwd/bwd + L1 + AdamW +
EMA (+ RCCL gradient all-reduce when N > 1).  Inputs: synthetic images resident in HBM
(no dataset / checkpoint is available offline).

A plain run sets up, warms up, times the K steps and prints the result line.  --dump-outputs DIR
also writes what the last timed step computed as DIR/<name>.npy (`dump_outputs`).  --full adds the
measurements that take runs of their own: DDIM sampling steps/s, the roofline of the dominant
kernel measured live with HIP events, the DP exchange timing, the eager reference-API step, and the
CPU oracle (the repo's restatement of the reference) timed on this host's cores.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# MI355X peaks (MI355X_MICROARCH.md, chip-level parameters): dense bf16 MFMA, HBM3E spec
PEAK_BF16_TFLOPS = 2500.0
PEAK_HBM_GBS = 8000.0
F_UNET_FWD_PER_IMG = 1.98671e9  # SURVEY.md §8(d), FlopCounterMode on the reference UNet


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results as DIR/<name>.npy (float32, seeded samples of the arenas)")
    ap.add_argument("--full", action="store_true",
                    help="also measure the GEMM roofline, DP exchange timing, DDIM rates, the eager reference-API "
                         "step and the CPU baseline (the --skip-* / --ddim-* options select among these)")
    ap.add_argument("--ddim-steps", type=int, default=200)
    ap.add_argument("--ddim-batch", type=int, default=8)
    ap.add_argument("--skip-ddim", action="store_true")
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-ref-api", action="store_true", help="skip the eager reference-API step timing")
    ap.add_argument("--bucket-mb", type=float, default=None,
                    help="DP: all-reduce pieces of at most this many MB (default ENCDIFF_DP_BUCKET_MB or coarse buckets)")
    ap.add_argument("--config", default="shapes3d", choices=["shapes3d", "celeba128"],
                    help="shapes3d: configs[1] (the bench line); celeba128: configs[4], builder-defined")
    return ap.parse_args()


def setup_dist(args):
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    # ENCDIFF_DP_FORCE=1 under torch.distributed.run --nproc-per-node 1: a one-rank RCCL group
    # and the full DP exchange path (trainer.HipTrainer.dp) on a single GPU
    if ws > 1 or (os.environ.get("ENCDIFF_DP_FORCE", "0") == "1" and "RANK" in os.environ):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # one process per GPU over RCCL ("nccl").  ENCDIFF_DIST_BACKEND=gloo rehearses the
        # DP path with several ranks sharing the GPUs of a smaller box (ranks wrap around).
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        backend = os.environ.get("ENCDIFF_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        return dist.get_rank(), ws
    torch.cuda.set_device(0)
    return 0, 1


WORKLOADS = {
    "shapes3d": ("training imgs/sec (node) Shapes3D 64x64 LDM",
                 "configs[1]: Shapes3D VQ-f4 16x16 latent LatentDiffusion training step (shapes3d-vq-4-16-encdiff)"),
    "celeba128": ("training imgs/sec (node) CelebA 128x128 LDM (builder-defined configs[4])",
                  "configs[4]: CelebA-shaped 128x128 VQ-f4 32x32 latent, model_channels 128, 40 concept tokens, "
                  "5-stage Encoder4, bf16 MFMA attention (ENCDIFF_ATTN_FP8=1: e4m3 scores at the S=1024 level)"),
}


def build_ldm(name="shapes3d"):
    import encdiff_amd  # noqa: F401
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    cfg = model_config(name)
    torch.manual_seed(0)
    ldm = instantiate_from_config(cfg)
    # The reference zero-initialises the UNet's output convolutions (zero_module: ResBlock
    # out_layers, SpatialTransformer proj_out, out): from that init eps_hat ~ 0 and most of the
    # backward carries zeros.  Re-draw them with PyTorch's default Conv2d / Linear init so the
    # timed step moves real data and loss_simple_last is not just E|N(0,1)|.
    for m in ldm.model.diffusion_model.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)) and not m.weight.detach().any():
            m.reset_parameters()
    return ldm.cuda(), cfg


def _copy_args(argp):
    import ctypes as C
    from encdiff_amd import _lib as L
    if not argp:
        return None
    a = L.GemmArgs()
    C.memmove(C.byref(a), argp, C.sizeof(L.GemmArgs))
    return a


def record_gemms(tr):
    """Every GEMM-family launch of one eager training step, in order: single GEMMs
    (encdiff_gemm, encdiff_gemm_ex), paired weight/input-gradient GEMMs with a deferred finalize
    riding along (encdiff_gemm_pair_ex, encdiff_gemm_pair_dx, encdiff_gemm_pair) and explicit
    finalizes (encdiff_gemm_finalize).  A finalize the step left to the GroupNorm / LayerNorm
    reading the output (gemm_ex / pair_dx deferrals) is recorded as part of its GEMM: the replay
    launches it, so the family keeps its full split-K cost.
    Returns [(kind, args...)]; `gemm_problems` lists the GEMM problems inside."""
    from encdiff_amd import _lib as L
    calls = []
    names = ("encdiff_gemm", "encdiff_gemm_ex", "encdiff_gemm_pair", "encdiff_gemm_pair_ex", "encdiff_gemm_pair_dx",
             "encdiff_gemm_finalize", "encdiff_wgrad_group_launch", "encdiff_st_wgrad_launch",
             "encdiff_st_wgrad_launch_nofold")
    orig = {n: getattr(L.lib, n) for n in names}

    def rec(name):
        def f(*a):
            stream = a[-1]
            if name in ("encdiff_gemm", "encdiff_gemm_ex"):
                calls.append(("gemm", _copy_args(a[0])))
            elif name == "encdiff_gemm_pair":
                calls.append(("pair_ex", _copy_args(a[0]), _copy_args(a[1]), None, 0))
            elif name in ("encdiff_gemm_pair_ex", "encdiff_gemm_pair_dx"):
                calls.append(("pair_ex", _copy_args(a[0]), _copy_args(a[1]), _copy_args(a[2]), a[3]))
            elif name == "encdiff_wgrad_group_launch":  # grouped weight gradients (blobs kept by the group)
                from encdiff_amd import ops
                calls.append(("group", a[0], a[1], [L.GemmArgs.from_buffer_copy(bytes(x)) for x in ops.GROUP_PROBS[a[0]]]))
            elif name.startswith("encdiff_st_wgrad_launch"):  # a fused transformer block's weight gradients
                # (replayed with its chunk fold, which the step carries in the GroupNorm backward's grid)
                from encdiff_amd import ops
                calls.append(("stwg", a[0], a[1], [L.GemmArgs.from_buffer_copy(bytes(x)) for x in ops.STWG_PROBS[a[0]]]))
            else:
                calls.append(("finalize", _copy_args(a[0])))
            return orig[name](*a[:-1], stream)
        return f
    for n in names:
        setattr(L.lib, n, rec(n))
    try:
        tr.step_eager()
    finally:
        for n in names:
            setattr(L.lib, n, orig[n])
    torch.cuda.synchronize()
    return calls


def gemm_problems(calls):
    out = []
    for c in calls:
        if c[0] == "gemm":
            out.append(c[1])
        elif c[0] == "pair_ex":
            out += [c[1], c[2]]
        elif c[0] in ("group", "stwg"):
            out += c[3]
    return out


def gemm_alg_bytes(a):
    """Algorithmic HBM bytes of one GEMM launch: each operand tensor read once (an im2col
    operand is its source image, not the 9x-expanded matrix), the output written once."""
    def src():
        pix = a.conv.batch * a.conv.h * a.conv.w
        # DOWN2 / STRIDE2 / K4S2 read a (2h, 2w) source, UP2 / K4S2_T an (h/2, w/2) one
        pix = pix * 4 if a.conv.resample in (1, 3, 4) else (pix // 4 if a.conv.resample in (2, 5) else pix)
        return 2.0 * pix * a.conv.cin
    abytes = src() if a.a_mode == 1 else 2.0 * a.M * a.K
    bbytes = src() if a.b_mode == 3 else 2.0 * a.N * a.K
    return abytes + bbytes + (2.0 if a.c_mode == 0 else 4.0) * a.M * a.N


def replay_gemms(calls, reps=1):
    import ctypes as C
    from encdiff_amd import _lib as L
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = lambda a: C.byref(a) if a is not None else None  # noqa: E731
    for _ in range(reps):
        for c in calls:
            if c[0] == "gemm":
                L.check(L.lib.encdiff_gemm(ref(c[1]), stream), "encdiff_gemm")
            elif c[0] == "pair_ex":
                L.check(L.lib.encdiff_gemm_pair_ex(ref(c[1]), ref(c[2]), ref(c[3]), c[4], stream), "pair_ex")
            elif c[0] == "group":
                L.check(L.lib.encdiff_wgrad_group_launch(c[1], c[2], stream), "wgrad_group")
            elif c[0] == "stwg":
                L.check(L.lib.encdiff_st_wgrad_launch(c[1], c[2], stream), "st_wgrad")
            else:
                L.check(L.lib.encdiff_gemm_finalize(ref(c[1]), stream), "finalize")


def kernel_roofline(tr, reps=10, config="shapes3d", batch=128):
    """Dominant kernel by time: the GEMM family (gemm_kernel<*> + its split-K finalize)
    that runs every conv / linear of the UNet, fwd + dgrad + wgrad.  The exact launches of
    one training step are recorded, captured into a HIP graph and replayed `reps` times
    between HIP events on the replay stream: achieved = algorithmic flops (sum 2*M*N*K)
    / GPU time, per launch averages reported beside it."""
    calls = record_gemms(tr)
    probs = gemm_problems(calls)
    flops = sum(2.0 * a.M * a.N * a.K for a in probs)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        replay_gemms(calls)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            replay_gemms(calls)
        g.replay()
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            g.replay()
        e1.record(s)
        s.synchronize()
    t_set = e0.elapsed_time(e1) / 1e3 / reps
    out = {"kernel": f"GEMM family (gemm_kernel / paired gemm2_kernel / WG3 + WGL weight-gradient grids / grouped weight "
                     f"gradients of the fused transformer backward (st_wgrad + fold) + split-K finalizes): {len(probs)} "
                     f"conv/linear GEMM problems of the step (UNet, VQ encoder, Encoder4; fwd+dgrad+wgrad) "
                     f"in {len(calls)} calls",
           "bound": "mfma", "achieved": flops / t_set / 1e12, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
           "frac": flops / t_set / 1e12 / PEAK_BF16_TFLOPS, "traffic": None,
           "avg_us": t_set / len(calls) * 1e6, "flops_per_launch": flops / len(calls),
           "launches_per_step": len(calls), "gemm_ms_per_step": t_set * 1e3,
           "alg_bytes_per_launch": sum(gemm_alg_bytes(a) for a in probs) / len(calls)}
    # HBM bytes per launch from the committed rocprofv3 PMC passes of THIS workload (configs[1]:
    # gemm_traffic.json, others gemm_traffic_<config>.json); null when that workload and batch
    # were not measured (a file measured on another config describes different GEMMs)
    fname = "gemm_traffic.json" if config == "shapes3d" else f"gemm_traffic_{config}.json"
    prof = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", fname)
    out["traffic_source"] = None
    if os.path.exists(prof):
        with open(prof) as f:
            pm = json.load(f)
        if int(pm.get("batch", 128)) == batch:
            out["traffic"] = pm.get("bytes_per_launch")
            out["traffic_source"] = f"profiles/{fname} ({pm.get('source', '')})"
    return out


def ddim_rate(ldm, B, S, eta=0.0):
    """DDIM steps/s of the whole captured S-step loop (one graph replay per sample() call)."""
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    unet = ldm.model.diffusion_model
    cond = torch.randn(B, unet.latent_unit * unet.context_dim, device="cuda")
    sampler = DDIMSampler(ldm)
    shape = (ldm.channels, ldm.image_size, ldm.image_size)
    x_T = torch.randn(B, *shape, device="cuda")
    with torch.no_grad():
        for _ in range(2):  # the first call replays the one-step graph, the second captures the loop
            sampler.sample(S, B, shape, cond, eta=eta, verbose=False, x_T=x_T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sampler.sample(S, B, shape, cond, eta=eta, verbose=False, x_T=x_T)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return S / dt


def log_images_time(ldm, N=8, S=200, eta=1.0):
    """The reference's logging workload (ddpm_enc.py:1473-1596 defaults: N=8, ddim_steps=200,
    ddim_eta=1.) with sample_swap (:1522-1535: every concept unit swapped, latent_unit x N rows):
    wall time of the COLD first call (one-step DDIM graphs captured and replayed for the 160-row
    swap batch and the 8-row sample batch, EMA scopes, VQ decodes), of the second call (captures
    the whole-loop graphs, ddim.LOOP_GRAPH_AFTER) and of a warm third call."""
    g = torch.Generator(device="cuda").manual_seed(7)
    batch = {"image": torch.rand(N, 64 * ldm.image_size // 16, 64 * ldm.image_size // 16, 3, device="cuda",
                                 generator=g) * 2 - 1}
    out = {}
    for k in ("cold_s", "second_s", "warm_s"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            log = ldm.log_images(batch, N=N, ddim_steps=S, ddim_eta=eta, sample_swap=True)
        torch.cuda.synchronize()
        out[k] = round(time.perf_counter() - t0, 4)
    lu = ldm.model.diffusion_model.latent_unit
    assert log["samples_swapping"].shape[0] == lu * N and log["samples"].shape[0] == N
    out.update(N=N, S=S, eta=eta, sample_swap_rows=lu * N, ddim_steps_total=S * 2,
               note="cold = first call (one-step graphs); second = whole-loop graph capture; warm = replay; "
                    "DDIM steps of both loops (swap + samples)")
    return out


def ref_api_time(config, B, steps=10, warmup=3):
    """The drop-in API path a reference-side Lightning loop drives (INTEGRATION.md §1;
    ddpm_enc.py:360-375 training_step, :399-401 on_train_batch_end, :1598-1639 optimizer), eager,
    on a model of its own: optimizer.zero_grad() + LatentDiffusion.training_step + loss.backward()
    + optimizer.step() + on_train_batch_end() per step.  Returns ms per step (host-synchronised
    wall time over `steps`; the batch is resident in HBM as in the graph bench)."""
    ldm, cfg = build_ldm(config)
    ldm.learning_rate = cfg.get("base_learning_rate", 2e-6) * B
    opt = ldm.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, (list, tuple)) else opt
    g = torch.Generator(device="cuda").manual_seed(11)
    res = 64 * ldm.image_size // 16
    batch = {"image": torch.rand(B, res, res, 3, device="cuda", generator=g) * 2 - 1}
    ldm.init_scale_factor(batch)

    def one(i):
        opt.zero_grad()
        loss = ldm.training_step(batch, i)
        loss.backward()
        opt.step()
        ldm.on_train_batch_end()
        return loss
    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = one(warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out = {"ms_per_step": ms, "imgs_per_s": B * 1e3 / ms, "batch": B, "steps": steps,
           "loss_last": float(loss), "note": "eager reference-API loop: zero_grad + training_step + "
                                             "backward + AdamW/EMA step + on_train_batch_end"}
    del ldm, opt
    torch.cuda.empty_cache()
    return out


def cpu_baseline(warmup=3, steps=50, ddim_steps=50, probe_steps=4):
    """BASELINE.md "CPU-baseline plan": the CPU oracle (the repo's fp32 restatement of the
    reference, pinned to reference fixtures) timed on this host's cores.
    Config 1: B=4 full training steps -- VQ encode + Encoder4 + q_sample + UNet fwd/bwd + L1 +
    AdamW + EMA -- x0 from the VQ encode of img ~ U(-1, 1), t ~ U{0..999}, eps ~ N(0, I), seed 1234,
    lr 4 * 2e-6; 3 warm-up + 50 timed steps.  DDIM: B=8, S=50, eta=0.
    Threads: a short probe over counts up to len(sched_getaffinity(0)) picks the fastest; the full
    measurement runs at that count (a B=4 step does not scale to dozens of threads: round 1's
    64-thread run was 3.7x slower than the reference on 8 vCPU)."""
    from oracle import encdiff_oracle as O
    avail = len(os.sched_getaffinity(0))
    counts = sorted({c for c in (1, 2, 4, 8, 16, 32) if c <= avail} | {min(avail, 64)})
    g = torch.Generator().manual_seed(1234)
    B = 4

    def batch():
        return (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1, torch.randint(0, 1000, (B,), generator=g),
                torch.randn(B, 3, 16, 16, generator=g))

    tr = O.OracleTrainer(O.build_plan(), lr=4 * 2e-6, vq=True)
    sweep = {}
    for c in counts:
        torch.set_num_threads(c)
        tr.step_images(*batch())
        t0 = time.perf_counter()
        for _ in range(probe_steps):
            tr.step_images(*batch())
        sweep[c] = B * probe_steps / (time.perf_counter() - t0)
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    for _ in range(warmup):
        tr.step_images(*batch())
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step_images(*batch())
    dt = time.perf_counter() - t0
    # DDIM B=8, S=50, eta=0 (ddim.py:114-207 restated by the oracle)
    plan = tr.plan
    P = {k: v.detach() for k, v in tr.P.items()}
    cond = torch.randn(8, 320, generator=g) * 0.5
    ac32 = O.sched_fp32(O.register_schedule())["alphas_cumprod"]
    xT = torch.randn(8, 3, 16, 16, generator=g)
    with torch.no_grad():
        t1 = time.perf_counter()
        O.ddim_sample(lambda x, ts: O.unet_forward(P, plan, x, ts, [cond]), xT, ddim_steps, 0.0, ac32)
        ddt = time.perf_counter() - t1
    return {"value": B * steps / dt, "unit": "imgs/s", "cores": best, "kind": "port",
            "sample": f"{warmup} warm-up + {steps} timed oracle training steps at batch {B} (fp32: VQ encode + "
                      f"Encoder4 + UNet fwd/bwd + AdamW + EMA) in {dt:.1f}s at {best} threads "
                      f"(of {avail} in the affinity mask)",
            "thread_sweep_imgs_per_s": {str(k): round(v, 3) for k, v in sweep.items()},
            "ddim_steps_per_sec": {"value": ddim_steps / ddt, "batch": 8, "S": ddim_steps, "eta": 0.0,
                                   "threads": best}}


DUMP_SAMPLE = 2 * 1024 * 1024  # elements kept of each arena-sized array (8 MB as float32)


def dump_outputs(tr, outdir, rank=0):
    """What the timed path left after its last step, as <outdir>/<name>.npy (float32; rank r > 0
    writes <name>.rank<r>.npy): `loss` (loss_simple, loss_vlb), `eps` (the denoiser output of
    the last batch), and of the flat arenas the step updates -- `grad` (the step's gradients),
    `params` (fp32 master weights after AdamW), `ema` -- of each the same DUMP_SAMPLE elements
    in every run (arena positions drawn from a fixed seed), about 25 MB in all."""
    import numpy as np
    torch.cuda.synchronize()
    os.makedirs(outdir, exist_ok=True)
    sfx = "" if rank == 0 else f".rank{rank}"

    def save(name, t):
        np.save(os.path.join(outdir, f"{name}{sfx}.npy"), t.detach().float().cpu().contiguous().numpy())

    def sample(flat):
        n = flat.numel()
        if n <= DUMP_SAMPLE:
            return flat
        idx = np.sort(np.random.default_rng(20240229).integers(0, n, DUMP_SAMPLE))
        return flat[torch.from_numpy(idx).to(flat.device)]

    a = tr.arena
    save("loss", tr.loss_buf[:2])
    save("eps", tr.eps())
    save("grad", sample(a.grad))
    save("params", sample(a.master))
    if a.ema is not None:
        save("ema", sample(a.ema))


def main():
    args = parse()
    rank, world = setup_dist(args)
    from encdiff_amd.trainer import HipTrainer, time_steps
    ldm, cfg = build_ldm(args.config)
    metric, workload = WORKLOADS[args.config]
    pool = {"shapes3d": 480000, "celeba128": 202599}[args.config]  # dataset sizes (CelebA: 202,599 images)
    tr = HipTrainer(ldm, args.batch, graph=not args.no_graph, pool_size=pool, bucket_mb=args.bucket_mb or 0.0)
    tr.init_scale_factor()
    tr.capture(warmup=3)
    for _ in range(args.warmup):
        tr.step()
    # marker kernels (torch's spin_kernel) bracket the timed region so a kernel trace can
    # be cut to it (tools/trace_window.py); they run outside the timed region
    torch.cuda._sleep(1000)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    dt = time_steps(tr, args.steps, events=ev)
    torch.cuda._sleep(1000)
    local_ms = ev[0].elapsed_time(ev[1]) / args.steps  # this rank's GPU time per step
    if args.dump_outputs:  # the state the last timed step left, before any further step moves it
        dump_outputs(tr, args.dump_outputs, rank)
    dp_info = None
    if tr.dp and args.full:  # exchange timing on extra steps (the timed ones carry no extra events)
        tr.dp_timing = True
        for _ in range(min(10, args.steps)):
            tr.step()
        tr.dp_timing = False
        dp_info = tr.dp_stats()
    dist_info = None
    if dist.is_initialized():
        t = torch.tensor([dt], device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
        # self-verifying multi-GPU line: what the process group itself reports (not the launcher's
        # WORLD_SIZE), and every rank's own GPU time per step (before the closing barrier)
        dvc = "cuda" if dist.get_backend() == "nccl" else "cpu"
        per = [torch.zeros(1, device=dvc) for _ in range(dist.get_world_size())]
        dist.all_gather(per, torch.tensor([local_ms], device=dvc))
        per = [round(float(x), 4) for x in per]
        dist_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                     "rank_gpu_ms_per_step": per, "rank_spread_ms": round(max(per) - min(per), 4),
                     "wall_ms_per_step_max_over_ranks": round(dt / args.steps * 1e3, 4)}
    imgs = args.batch * world * args.steps
    value = imgs / dt
    loss = tr.loss()
    extra = {}
    # every rank (its recording step runs the DP exchange)
    roof = kernel_roofline(tr, config=args.config, batch=args.batch) if args.full else None
    if rank == 0:
        if roof is not None:
            extra["roofline"] = roof
        if dp_info is not None:
            extra["dp"] = dp_info
        if dist_info is not None:
            extra["dist"] = dist_info
        f_step = 3 * F_UNET_FWD_PER_IMG * args.batch  # configs[1]'s UNet; other configs: see the GEMM roofline
        if args.config == "shapes3d":
            extra["step_roofline"] = {"bound": "mfma", "unit": "TFLOP/s",
                                      "achieved": f_step * args.steps / dt / 1e12,
                                      "peak": PEAK_BF16_TFLOPS,
                                      "frac": f_step * args.steps / dt / 1e12 / PEAK_BF16_TFLOPS,
                                      "flops_per_img": 3 * F_UNET_FWD_PER_IMG}
        if args.full and not args.skip_ddim:
            # DDIM steps/s at (B=8, S=200, eta=0) and (B=128, S=200, eta=1)
            extra["ddim_steps_per_sec"] = {"value": ddim_rate(ldm, args.ddim_batch, args.ddim_steps),
                                           "batch": args.ddim_batch, "S": args.ddim_steps, "eta": 0.0}
            extra["ddim_steps_per_sec_b128"] = {"value": ddim_rate(ldm, 128, args.ddim_steps, eta=1.0),
                                                "batch": 128, "S": args.ddim_steps, "eta": 1.0}
            if args.config == "shapes3d":
                extra["ddim_log_images_s"] = log_images_time(ldm)
        if args.full and not args.skip_ref_api and world == 1:
            r = ref_api_time(args.config, args.batch)
            extra["ref_api_ms_per_step"] = r["ms_per_step"]
            extra["ref_api"] = r
        if args.full and not args.skip_cpu and world == 1 and args.config == "shapes3d":  # CPU baseline: N=1, configs[1]
            extra["cpu_baseline"] = cpu_baseline()
    if rank == 0:
        out = {"metric": metric, "value": value, "unit": "imgs/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "bf16",
               "data": "synthetic (uint8 images resident in HBM; random init, zero-init UNet output convs re-drawn)",
               "config": {"workload": workload, "global_batch": args.batch * world,
                          "per_gpu_batch": args.batch, "parallelism": f"dp{world}",
                          "graph": not args.no_graph},
               "loss_simple_last": loss}
        out.update(extra)
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
