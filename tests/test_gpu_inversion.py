"""DDIM inversion through the public API (DDIMSamplerAttn.ddim_loop / ddim_inversion / sample,
LatentDiffusion.sample_log_attn / log_images) on the eager, the one-step-graph and the
whole-loop-graph path.  Recipe-weight Shapes3D model, B = 2, S = 10.

Bounds.  Against the reference (tests/golden/ddim_inversion.npz, its fp32 CPU loop): for every latent
k = 1 .. 10 of the trajectory rel-L2 <= max(3e-2, 2 x rel-L2(reference bf16-autocast loop, reference
fp32 loop) at k).  3e-2 is the project's DDIM bound; with the recipe weights this loop amplifies
rounding differences (the reference's own bf16 loop ends 3.84e-2 from its fp32 loop), and two bf16
realisations of it differ by about twice one's distance from fp32 -- the rule of
test_gpu_vq_decode.py.  Teacher-forced (one step from the fixture's latent k): rel-L2 <= 3e-2, no
accumulation.  Captured against eager: the fp32 rule of tests/elementwise_restate.py with the eager run
as the reference and no additive floor (same_rule of test_gpu_sampling.py).  For the log_images row the
rule is applied to the latent that is decoded into inversion_reconstruction, and the image is tied to
that latent by the decode call itself: the torch first stage between them is not bit-reproducible.

Measured on MI355X: see DESIGN.md §1.
"""
import os

import numpy as np
import pytest
import torch

from elementwise_restate import f32_excess, same_bits

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 16, 16)
S = 10


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
    # log_images samples inside ema_scope(): give the EMA the recipe weights too.  The shadow taken at
    # construction holds the zero-initialised output conv, under which eps is 0 and neither the
    # conditioning nor the UNet would take part in the rows tested below.
    from encdiff_amd.ldm.modules.ema import LitEma
    m.model_ema = LitEma(m.model)
    return m.cuda()


@pytest.fixture(scope="module")
def fx(golden_dir):
    f = np.load(os.path.join(golden_dir, "ddim_inversion.npz"))
    d = {k: (torch.tensor(f[k]).cuda() if f[k].ndim else int(f[k])) for k in f.files}
    assert d["steps"] == S and d["all_latent"].shape == (S + 1,) + SHAPE
    return d


def same_rule(out, ref, what):
    ex, i, worst = f32_excess(out, ref.double(), 0.0)
    print(f"{what}: largest |captured - eager| {worst:.3e}, excess over 2^-22 |ref| {ex:.3e}")
    assert ex <= 0, (what, ex, i, worst)


def sampler(ldm, path, monkeypatch, cls="DDIMSamplerAttn"):
    from encdiff_amd.ldm.models.diffusion import ddim as D
    # "loop": the first call captures the whole loop; "step": every call replays the one-step graph
    monkeypatch.setattr(D, "LOOP_GRAPH_AFTER", 0)
    monkeypatch.setattr(D, "GRAPH_MAX_STEPS", 2 if path == "step" else 256)
    return getattr(D, cls)(ldm, use_graph=path != "eager")


def kinds(s):
    return sorted(k[0] for k in s._graphs)


def took(s, path):
    assert kinds(s) == ([] if path == "eager" else ["inv_" + path]), "the sampler did not take the expected path"


def eager_loop(ldm, x0, cond):
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSamplerAttn
    with torch.no_grad():
        return DDIMSamplerAttn(ldm, use_graph=False).ddim_loop(x0, cond, S)[0]


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("path", ["eager", "step", "loop"])
def test_trajectory_matches_reference(ldm, fx, path, monkeypatch):
    s = sampler(ldm, path, monkeypatch)
    x0 = fx["x0"].clone()
    with torch.no_grad():
        lat, inter = s.ddim_loop(x0, fx["cond"], S)
        zT, inter2 = s.ddim_inversion(x0, fx["cond"], S)
    took(s, path)
    assert inter == {"context": []} and inter2 == {"context": []}
    assert len(lat) == S + 1 and lat[0] is x0 and same_bits(x0, fx["x0"]), "all_latent[0] is the caller's tensor"
    assert same_bits(zT, lat[-1])
    assert np.array_equal(np.asarray(s.ddim_timesteps), fx["ddim_timesteps"].cpu().numpy())
    ours = [rel(lat[k], fx["all_latent"][k]) for k in range(1, S + 1)]
    ref16 = [rel(fx["all_latent_bf16"][k], fx["all_latent"][k]) for k in range(1, S + 1)]
    print(f"inversion {path}: rel-L2 vs the reference fp32 loop, k = 1 .. {S}")
    print("  ours          " + " ".join(f"{v:.3e}" for v in ours))
    print("  reference bf16 " + " ".join(f"{v:.3e}" for v in ref16))
    for k in range(S):
        assert ours[k] <= max(3e-2, 2 * ref16[k]), (path, k + 1, ours[k], ref16[k])


@pytest.mark.parametrize("k", [0, 4, 9])
def test_teacher_forced_step_matches_reference(ldm, fx, k):
    """One inversion step from the fixture's latent k: the UNet, then the step kernel."""
    from encdiff_amd import ops
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSamplerAttn
    s = DDIMSamplerAttn(ldm, use_graph=False)
    s.make_schedule(S, ddim_eta=0., verbose=False)
    x = fx["all_latent"][k].contiguous()
    t = torch.full((2,), int(s.ddim_timesteps[k]), device="cuda", dtype=torch.long)
    with torch.no_grad():
        e_t = ldm.apply_model(x, t, fx["cond"]).float().contiguous()
        xn = torch.empty_like(x)
        ops.ddim_invert_step(x, e_t, (float(s.ddim_alphas[k]), float(s.ddim_alphas_next[k])), xn)
    r, re = rel(xn, fx["all_latent"][k + 1]), rel(e_t, fx["eps"][k])
    print(f"teacher-forced step k={k}: rel-L2 next latent {r:.3e}, eps {re:.3e}")
    assert r <= 3e-2


# ------------------------------------------------------------------ captured against eager, replay
@pytest.mark.parametrize("path", ["step", "loop"])
def test_captured_equals_eager_and_replay(ldm, fx, path, monkeypatch):
    s = sampler(ldm, path, monkeypatch)
    calls = [(fx["x0"], fx["cond"]), (fx["x0"].flip(0) * 0.5, fx["cond"].flip(0)), (fx["x0"], fx["cond"])]
    outs, kept = [], []
    for i, (x0, cond) in enumerate(calls):
        with torch.no_grad():
            lat, _ = s.ddim_loop(x0, cond, S)
        ref = eager_loop(ldm, x0, cond)
        assert len(lat) == len(ref) == S + 1
        for k in range(1, S + 1):
            same_rule(lat[k], ref[k], f"inversion {path} call {i}: latent {k}")
        outs.append(lat)
        kept.append([v.clone() for v in lat])
    took(s, path)
    assert len(s._graphs) == 1, "the later calls replay the first call's graph"
    for i in range(3):  # a later call leaves an earlier call's result as it was
        assert all(same_bits(a, b) for a, b in zip(outs[i], kept[i])), i
    assert rel(outs[1][-1], outs[0][-1]) > 1e-2
    assert all(same_bits(a, b) for a, b in zip(outs[0][1:], outs[2][1:]))


# ------------------------------------------------------------------ sampling and inversion on one sampler
@pytest.mark.parametrize("first", ["sample", "invert"])
def test_sampling_and_inversion_graphs_do_not_collide(ldm, fx, first, monkeypatch):
    s = sampler(ldm, "loop", monkeypatch)
    plain = sampler(ldm, "loop", monkeypatch, cls="DDIMSampler")
    xT = fx["all_latent"][S].contiguous()
    got = {}
    with torch.no_grad():
        for what in ([first] + [w for w in ("sample", "invert") if w != first]) * 2:  # capture, then replay
            if what == "sample":
                got[what], inter = s.sample(S, 2, SHAPE[1:], fx["cond"], eta=0., verbose=False, x_T=xT)
                assert inter["context"] == [] and list(inter) == ["x_inter", "pred_x0", "context"]
            else:
                got[what] = s.ddim_loop(fx["x0"], fx["cond"], S)[0]
        want, winter = plain.sample(S, 2, SHAPE[1:], fx["cond"], eta=0., verbose=False, x_T=xT)
    assert kinds(s) == ["inv_loop", "loop"] and kinds(plain) == ["loop"]
    assert "context" not in winter
    assert same_bits(got["sample"], want), "DDIMSamplerAttn.sample takes DDIMSampler's path"
    ref = eager_loop(ldm, fx["x0"], fx["cond"])
    for k in range(1, S + 1):
        same_rule(got["invert"][k], ref[k], f"inversion after/before sampling ({first} first): latent {k}")


@pytest.mark.parametrize("path", ["step", "loop"])
def test_inversion_feeds_sampling(ldm, fx, path, monkeypatch):
    """ddim_inversion's output handed straight to sample(x_T=...) against the same with clones in
    between: a buffer shared by the two graphs would show."""
    s = sampler(ldm, path, monkeypatch)
    with torch.no_grad():
        zT, _ = s.ddim_inversion(fx["x0"], fx["cond"], S)
        keep = zT.clone()
        direct, _ = s.sample(S, 2, SHAPE[1:], fx["cond"], eta=0., verbose=False, x_T=zT)
        assert same_bits(zT, keep), "sampling changed the inversion's returned latent"
        zT2, _ = s.ddim_inversion(fx["x0"].clone(), fx["cond"].clone(), S)
        cloned, _ = s.sample(S, 2, SHAPE[1:], fx["cond"].clone(), eta=0., verbose=False, x_T=zT2.clone())
    assert kinds(s) == sorted(["inv_" + path, path])
    assert same_bits(zT2, keep) and same_bits(direct, cloned)
    assert torch.isfinite(direct).all()


# ------------------------------------------------------------------ model level
def test_sample_log_attn(ldm, fx):
    xT = fx["all_latent"][S].contiguous()
    with torch.no_grad():
        a, ai = ldm.sample_log_attn(cond=fx["cond"], batch_size=2, ddim=True, ddim_steps=S, eta=0., x_T=xT)
        b, bi = ldm.sample_log(cond=fx["cond"], batch_size=2, ddim=True, ddim_steps=S, eta=0., x_T=xT)
    assert ldm.ddim_attn_sampler() is ldm.ddim_attn_sampler() and ldm.ddim_attn_sampler() is not ldm.ddim_sampler()
    assert same_bits(a, b)
    assert ai["context"] == [] and "context" not in bi
    for key in ("x_inter", "pred_x0"):
        assert len(ai[key]) == len(bi[key]) and all(same_bits(u, v) for u, v in zip(ai[key], bi[key])), key
    with pytest.raises(NotImplementedError, match="openaimodel_enc.py:712"):
        ldm.sample_log_attn(cond=fx["cond"], batch_size=2, ddim=True, ddim_steps=S, return_context=True)
    with torch.no_grad():  # ddim=False reaches LatentDiffusion.sample (the ancestral loop)
        samples, inter = ldm.sample_log_attn(cond=fx["cond"], batch_size=2, ddim=False, ddim_steps=None, timesteps=4)
    assert samples.shape == SHAPE and torch.isfinite(samples).all()
    assert isinstance(inter, list) and len(inter) == 3 and torch.equal(inter[-1], samples)


def test_log_images_inversion_rows(ldm, monkeypatch):
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSampler, DDIMSamplerAttn
    g = torch.Generator().manual_seed(12)
    img = (torch.rand(2, 64, 64, 3, generator=g) * 2 - 1).cuda()
    kw = dict(N=2, ddim_steps=S, ddim_eta=0., plot_diffusion_rows=False, sample_swap=True)
    new = {"inversion_reconstruction", "samples_swap_inverted"}
    assert ldm.log_images_inversion is False
    with torch.no_grad():
        base = ldm.log_images({"image": img}, **kw)
    assert not (set(base) & new) and {"reconstruction", "samples_swapping"} <= set(base)
    monkeypatch.setattr(ldm, "log_images_inversion", True, raising=False)
    seen = []  # (z, c) of each log_images call: the encoders are not bit-reproducible from call to call
    decoded = []  # (latent, image, further arguments) of every decode_first_stage call
    inner, inner_dec = ldm.get_input, ldm.decode_first_stage

    def recording(*args, **kwargs):
        out = inner(*args, **kwargs)
        seen.append((out[0].clone(), out[1].clone()))
        return out

    def recording_dec(z, *args, **kwargs):
        out = inner_dec(z, *args, **kwargs)
        decoded.append((z.clone(), out, args, kwargs))
        return out

    monkeypatch.setattr(ldm, "get_input", recording)
    monkeypatch.setattr(ldm, "decode_first_stage", recording_dec)
    with torch.no_grad():
        log = ldm.log_images({"image": img}, **kw)
        noswap = ldm.log_images({"image": img}, **{**kw, "sample_swap": False})
    monkeypatch.setattr(ldm, "get_input", inner)
    monkeypatch.setattr(ldm, "decode_first_stage", inner_dec)
    assert len(seen) == 2
    assert set(log) == set(base) | new
    assert set(noswap) == (set(base) | {"inversion_reconstruction"}) - {"samples_swapping"}
    assert log["inversion_reconstruction"].shape == log["reconstruction"].shape == (2, 3, 64, 64)
    assert log["samples_swap_inverted"].shape == log["samples_swapping"].shape
    for k in new:
        assert torch.isfinite(log[k]).all(), k
    assert same_bits(log["inputs"], base["inputs"])
    # The manually composed pipeline, eager, from each call's own (z, c).  The captured-versus-eager
    # rule is applied to the latent that log_images hands to decode_first_stage: everything up to there
    # runs on this project's kernels, where the two paths launch the same arithmetic.  The decode
    # itself is the torch first stage, which is not bit-reproducible from call to call on identical
    # input (a whole-suite run met 2.4e-6 between two decodes of latents that cannot differ), so the
    # image is tied to that latent by the call itself: it is the object decode_first_stage returned
    # for it, called with no other argument.
    for (z, c), got, what in zip(seen, (log, noswap), ("first call", "replayed")):
        call = [(zl, a, k) for zl, im, a, k in decoded if im is got["inversion_reconstruction"]]
        assert len(call) == 1 and call[0][1:] == ((), {}), "inversion_reconstruction is decode_first_stage(latent)"
        lat = call[0][0]
        with torch.no_grad():
            with ldm.ema_scope():
                zT, _ = DDIMSamplerAttn(ldm, use_graph=False).ddim_inversion(z, c, S)
                rec, _ = DDIMSampler(ldm, use_graph=False).sample(S, 2, SHAPE[1:], c, eta=0., verbose=False, x_T=zT)
                eps = ldm.apply_model(z, torch.full((2,), 1, device="cuda", dtype=torch.long), c)
            want = ldm.decode_first_stage(rec)
        assert eps.abs().max().item() > 1e-3, "the UNet takes part: eps is not 0 under the EMA weights"
        same_rule(lat, rec, f"latent behind inversion_reconstruction vs the eager pipeline, {what}")
        print(f"{what}: decoded image vs the decode of the eager latent: max |d| "
              f"{(got['inversion_reconstruction'] - want).abs().max().item():.3e}, rel-L2 "
              f"{rel(got['inversion_reconstruction'], want):.3e}")
