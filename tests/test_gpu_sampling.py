"""Inpainting, quantised-x0 and ancestral sampling through the public API (DDIMSampler,
LatentDiffusion.p_sample_loop / progressive_denoising / sample_log / log_images) on the captured
and the eager paths.

Bounds.  Against the reference (tests/golden/sampling.npz, its CPU noise stream injected): rel-L2
<= 3e-2 on the final sample and the last intermediate, the project's DDIM bound for bf16
activations against the fp32 reference.  Captured against eager: the fp32 rule of
tests/elementwise_restate.py with the eager run as the reference and no additive floor -- both
paths launch the same kernels on the same UNet output, so nothing but the rule's 2^-22 |ref| is
allowed.  Quantised DDIM: pred_x0 is bitwise made of codebook rows; against the torch quantiser
(one step, same x and e_t) indices agree wherever the fp64 gap between the best and the
second-best squared distance is >= 1e-4 max(1, best), the excluded rows at most 2 %.

Measured on MI355X (rel-L2 vs the reference, final sample / last intermediate): see DESIGN.md §1.
"""
import os

import numpy as np
import pytest
import torch

from elementwise_restate import f32_excess

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 16, 16)


def rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ldm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    from oracle import encdiff_oracle as O
    m = instantiate_from_config(model_config("shapes3d"))
    with torch.no_grad():
        for n, p in m.model.diffusion_model.named_parameters():
            p.copy_(O.recipe_tensor(n, tuple(p.shape)))
        for n, p in m.cond_stage_model.named_parameters():
            p.copy_(O.recipe_tensor("cond." + n, tuple(p.shape)))
        for n, p in m.first_stage_model.named_parameters():
            p.copy_(O.recipe_tensor("vq." + n, tuple(p.shape)))
    return m.cuda()


@pytest.fixture(scope="module")
def fx(golden_dir):
    f = np.load(os.path.join(golden_dir, "sampling.npz"))
    return {k: (torch.tensor(f[k]).cuda() if f[k].ndim else int(f[k])) for k in f.files}


def ref_draws(n, seed):
    """The reference's CPU noise stream as tools/gen_golden_sampling.py consumed it:
    torch.manual_seed(seed), then one torch.randn(x.shape) per draw."""
    torch.manual_seed(seed)
    return torch.stack([torch.randn(SHAPE) for _ in range(n)]).cuda()


def same_rule(out, ref, what):
    ex, i, worst = f32_excess(out, ref.double(), 0.0)
    print(f"{what}: largest |captured - eager| {worst:.3e}, excess over 2^-22 |ref| {ex:.3e}")
    assert ex <= 0, (what, ex, i, worst)


def sampler(ldm, path, monkeypatch):
    from encdiff_amd.ldm.models.diffusion import ddim as D
    # "loop": the first call captures the whole loop; "step": every call replays the one-step graph
    monkeypatch.setattr(D, "LOOP_GRAPH_AFTER", 0)
    monkeypatch.setattr(D, "GRAPH_MAX_STEPS", 2 if path == "step" else 256)
    s = D.DDIMSampler(ldm, use_graph=path != "eager")
    return s


def took(s, path):
    if path == "eager":
        assert not s._graphs
    else:
        assert [k[0] for k in s._graphs] == [path], "the sampler did not take the expected graph path"


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_p_sample_loop_matches_reference(ldm, fx, graph, monkeypatch):
    monkeypatch.setattr(ldm, "ancestral_use_graph", graph, raising=False)
    nz = ref_draws(fx["steps"], fx["seed"])
    with torch.no_grad():
        out, inter = ldm.p_sample_loop(fx["cond"], SHAPE, return_intermediates=True, x_T=fx["xT"], verbose=False,
                                       timesteps=fx["steps"], log_every_t=fx["log_every_t"], normals_sequence=nz)
    assert bool(getattr(ldm, "_anc_graphs", None)) or not graph
    got = torch.stack(inter)
    assert got.shape == fx["anc_inter"].shape and torch.equal(got[0], fx["xT"])
    r, rl = rel(out, fx["anc_samples"]), rel(got[-1], fx["anc_inter"][-1])
    print(f"p_sample_loop graph={graph}: rel-L2 samples {r:.3e}, last intermediate {rl:.3e}, all logged "
          f"{[round(rel(a, b), 5) for a, b in zip(got[1:], fx['anc_inter'][1:])]}")
    assert r <= 3e-2 and rl <= 3e-2


@pytest.mark.parametrize("graph", [True, False], ids=["captured", "eager"])
def test_progressive_denoising_matches_reference(ldm, fx, graph, monkeypatch):
    monkeypatch.setattr(ldm, "ancestral_use_graph", graph, raising=False)
    nz = ref_draws(fx["steps"], fx["seed"])
    with torch.no_grad():
        out, x0s = ldm.progressive_denoising(fx["cond"], SHAPE, verbose=False, x_T=fx["xT"], start_T=fx["steps"],
                                             log_every_t=fx["log_every_t"], normals_sequence=nz)
    got = torch.stack(x0s)
    assert got.shape == fx["prog_x0"].shape
    r, rl = rel(out, fx["prog_samples"]), rel(got[-1], fx["prog_x0"][-1])
    print(f"progressive_denoising graph={graph}: rel-L2 samples {r:.3e}, last x0_partial {rl:.3e}, all logged "
          f"{[round(rel(a, b), 5) for a, b in zip(got, fx['prog_x0'])]}")
    assert r <= 3e-2 and rl <= 3e-2


def masked_ddim(s, fx, eta, cond=None, xT=None, mask=None, x0=None, draws=None, **kw):
    draws = ref_draws(2 * fx["steps"], fx["seed"]) if draws is None else draws
    with torch.no_grad():  # per step the re-noise was drawn first, the step noise second
        return s.sample(fx["steps"], 2, SHAPE[1:], fx["cond"] if cond is None else cond, eta=float(eta),
                        verbose=False, x_T=fx["xT"] if xT is None else xT, mask=fx["mask"] if mask is None else mask,
                        x0=fx["x0"] if x0 is None else x0, mask_normals_sequence=draws[0::2],
                        normals_sequence=draws[1::2], **kw)


@pytest.mark.parametrize("path", ["step", "loop", "eager"])
@pytest.mark.parametrize("eta", [0, 1])
def test_masked_ddim_matches_reference(ldm, fx, eta, path, monkeypatch):
    s = sampler(ldm, path, monkeypatch)
    out, inter = masked_ddim(s, fx, eta)
    took(s, path)
    r, rp = rel(out, fx[f"mddim_samples_eta{eta}"]), rel(inter["pred_x0"][-1], fx[f"mddim_pred_x0_last_eta{eta}"])
    print(f"masked ddim eta{eta} {path}: rel-L2 samples {r:.3e}, last pred_x0 {rp:.3e}")
    assert r <= 3e-2 and rp <= 3e-2
    # the final sample is not blended: the known region has moved off q_sample(x0)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) >= 2


# ------------------------------------------------------------------ captured against eager
@pytest.mark.parametrize("path", ["step", "loop"])
def test_masked_ddim_captured_equals_eager_and_reuse(ldm, fx, path, monkeypatch):
    """One captured sampler, two calls: the second with another x_T, conditioning, mask (per-channel)
    and x0 must match a fresh eager run (the mask and x0 are buffers of the cache entry)."""
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    s = sampler(ldm, path, monkeypatch)
    g = torch.Generator().manual_seed(17)
    m2 = (torch.rand(2, 1, 16, 16, generator=g) < 0.5).float().cuda()
    calls = [dict(), dict(cond=fx["cond"].flip(0), xT=fx["xT"] * 0.5, mask=m2, x0=fx["x0"].flip(0) * 1.5),
             dict()]
    outs = []
    for i, kw in enumerate(calls):
        o, oi = masked_ddim(s, fx, 1, **kw)
        e, ei = masked_ddim(DDIMSampler(ldm, use_graph=False), fx, 1, **kw)
        same_rule(o, e, f"masked ddim {path} call {i}: samples")
        same_rule(oi["pred_x0"][-1], ei["pred_x0"][-1], f"masked ddim {path} call {i}: last pred_x0")
        same_rule(oi["x_inter"][-1], ei["x_inter"][-1], f"masked ddim {path} call {i}: last x_inter")
        outs.append(o)
    took(s, path)
    assert rel(outs[0], outs[1]) > 1e-2 and torch.equal(outs[0], outs[2])
    # a (B, C, H, W) mask is another cache entry
    m3 = m2.expand(2, 3, 16, 16).contiguous()
    o, _ = masked_ddim(s, fx, 1, mask=m3)
    e, _ = masked_ddim(DDIMSampler(ldm, use_graph=False), fx, 1, mask=m2)
    same_rule(o, e, f"masked ddim {path}: per-channel mask")
    assert len(s._graphs) == 2


def test_ancestral_captured_equals_eager_and_reuse(ldm, fx, monkeypatch):
    nz = ref_draws(2 * fx["steps"], fx["seed"])
    g = torch.Generator().manual_seed(18)
    m2 = (torch.rand(2, 1, 16, 16, generator=g) < 0.5).float().cuda()
    calls = [dict(cond=fx["cond"], x_T=fx["xT"]),
             dict(cond=fx["cond"].flip(0), x_T=fx["xT"] * 0.5),
             dict(cond=fx["cond"], x_T=fx["xT"], mask=fx["mask"], x0=fx["x0"], mask_normals_sequence=nz[1::2]),
             dict(cond=fx["cond"].flip(0), x_T=fx["xT"] * 0.5, mask=m2, x0=fx["x0"] * 1.5,
                  mask_normals_sequence=nz[1::2])]
    for i, kw in enumerate(calls):
        res = {}
        for graph in (True, False):
            monkeypatch.setattr(ldm, "ancestral_use_graph", graph, raising=False)
            with torch.no_grad():
                res[graph] = ldm.p_sample_loop(kw["cond"], SHAPE, return_intermediates=True, verbose=False,
                                               timesteps=fx["steps"], log_every_t=fx["log_every_t"],
                                               normals_sequence=nz[0::2],
                                               **{k: v for k, v in kw.items() if k != "cond"})
        same_rule(res[True][0], res[False][0], f"ancestral call {i}: samples")
        for j, (a, b) in enumerate(zip(res[True][1], res[False][1])):
            same_rule(a, b, f"ancestral call {i}: intermediate {j}")
        assert len(res[True][1]) == len(res[False][1]) == 5
    assert len(ldm._anc_graphs) >= 2


# ------------------------------------------------------------------ quantised DDIM
def code_index(px0, E):
    """Index of the codebook row each pixel vector equals bitwise (-1: none)."""
    r = px0.permute(0, 2, 3, 1).reshape(-1, px0.shape[1])
    hit = (r[:, None, :] == E[None]).all(-1)
    return torch.where(hit.any(1), hit.float().argmax(1), torch.full((r.shape[0],), -1, device=r.device))


def test_quantised_ddim(ldm, fx, monkeypatch):
    """S = 4, B = 2, eta 0 (S = 3 does not exist on a 1000-step schedule: the uniform DDIM
    discretisation of util.py steps by 1000 // 3 and ends on timestep 1000, out of range)."""
    E = ldm.first_stage_model.quantize.embedding.weight.detach()
    res = {}
    for path in ("step", "loop", "eager"):
        s = sampler(ldm, path, monkeypatch)
        with torch.no_grad():
            out, inter = s.sample(4, 2, SHAPE[1:], fx["cond"], eta=0.0, verbose=False, x_T=fx["xT"], quantize_x0=True,
                                  log_every_t=1)
        took(s, path)
        assert len(inter["pred_x0"]) == 5  # x_T, then every step
        idx = torch.stack([code_index(p, E) for p in inter["pred_x0"][1:]])
        assert (idx >= 0).all(), f"{path}: a pred_x0 pixel is not a codebook row"
        res[path] = (out, idx)
        assert torch.isfinite(out).all()
    for path in ("step", "loop"):
        assert torch.equal(res[path][1], res["eager"][1]), f"{path}: indices differ from the eager run"
        assert torch.equal(res[path][0], res["eager"][0]), f"{path}: samples differ from the eager run"


def test_quantised_step_agrees_with_torch_quantiser(ldm, fx):
    """One step from the same x and e_t: the kernel's indices vs first_stage_model.quantize (the
    parent's branch of p_sample_ddim), under the gap rule."""
    from encdiff_amd import ops
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSampler
    s = DDIMSampler(ldm, use_graph=False)
    s.make_schedule(ddim_num_steps=4, ddim_eta=0.0, verbose=False)
    index = 3
    x = fx["xT"]
    t = torch.full((2,), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
    E = ldm.first_stage_model.quantize.embedding.weight.detach()
    with torch.no_grad():
        e_t = ldm.apply_model(x, t, fx["cond"]).float().contiguous().clone()
        a_t, a_prev = float(s.ddim_alphas[index]), float(s.ddim_alphas_prev[index])
        sigma, s1 = float(s.ddim_sigmas[index]), float(s.ddim_sqrt_one_minus_alphas[index])
        idx = torch.full((2 * 256,), -1, device="cuda", dtype=torch.int32)
        xp, px0 = torch.empty_like(x), torch.empty_like(x)
        ops.ddim_step_quantized(x, e_t, None, (a_t, a_prev, sigma, s1), E, xp, px0, idx=idx)
        pred = (x - s1 * e_t) / np.sqrt(a_t)
        zq, _, (_, _, tidx) = ldm.first_stage_model.quantize(pred)
    p64 = (x.double() - torch.tensor(s1, dtype=torch.float32).double() * e_t.double()) / \
        torch.tensor(a_t, dtype=torch.float32).double().sqrt()
    d = ((p64.permute(0, 2, 3, 1).reshape(-1, 3)[:, None, :] - E.double()[None]) ** 2).sum(-1)
    b2 = torch.topk(d, 2, dim=1, largest=False).values
    keep = (b2[:, 1] - b2[:, 0]) >= 1e-4 * b2[:, 0].clamp_min(1.0)
    excluded = (~keep).sum().item()
    print(f"one quantised step: {excluded} of {keep.numel()} rows excluded, "
          f"{(idx.long() != tidx.reshape(-1)).sum().item()} indices differ from the torch quantiser in all")
    assert excluded <= 0.02 * keep.numel()
    assert torch.equal(idx.long()[keep], tidx.reshape(-1)[keep])
    assert torch.equal(idx.long()[keep], d.argmin(1)[keep])
    assert torch.equal(code_index(px0, E), idx.long())  # the kernel writes the code itself


# ------------------------------------------------------------------ unmasked sampling, log_images
def test_sample_log_without_ddim(ldm, fx):
    with torch.no_grad():
        samples, inter = ldm.sample_log(cond=fx["cond"], batch_size=2, ddim=False, ddim_steps=None, timesteps=4)
    assert samples.shape == SHAPE and torch.isfinite(samples).all()
    assert isinstance(inter, list) and len(inter) == 3  # x_T, i = 3 (the first step), i = 0
    assert all(v.shape == SHAPE for v in inter) and torch.equal(inter[-1], samples)


def test_log_images_full_rows(ldm, monkeypatch):
    g = torch.Generator().manual_seed(12)
    img = (torch.rand(2, 64, 64, 3, generator=g) * 2 - 1).cuda()
    kw = dict(N=2, ddim_steps=2, plot_diffusion_rows=False, plot_denoise_rows=True)
    assert ldm.log_images_full is False
    with torch.no_grad():
        base = ldm.log_images({"image": img}, **kw)
    assert set(base) == {"inputs", "reconstruction", "samples"}  # the parent's keys
    monkeypatch.setattr(ldm, "log_images_full", True, raising=False)
    monkeypatch.setattr(ldm, "log_every_t", 2)
    monkeypatch.setattr(ldm, "_progressive_start_T", 4, raising=False)
    with torch.no_grad():
        log = ldm.log_images({"image": img}, **kw)
    new = {"samples_x0_quantized", "samples_inpainting", "samples_outpainting", "mask", "denoise_row",
           "progressive_row"}
    assert set(log) == set(base) | new
    for k in ("samples", "samples_x0_quantized", "samples_inpainting", "samples_outpainting"):
        assert log[k].shape == (2, 3, 64, 64), k
    want = torch.ones(2, 1, 16, 16, device="cuda")
    want[:, :, 4:12, 4:12] = 0
    assert torch.equal(log["mask"], want)
    assert log["denoise_row"].shape == (3, 2, 3, 64, 64)      # x_T and the 2 DDIM steps (log_every_t = 100)
    assert log["progressive_row"].shape == (3, 2, 3, 64, 64)  # i = 3, 2, 0 of start_T = 4 at log_every_t = 2
    for k, v in log.items():
        assert torch.isfinite(v).all(), k
