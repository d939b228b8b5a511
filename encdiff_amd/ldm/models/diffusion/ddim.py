"""DDIMSampler -- mirror of ldm/models/diffusion/ddim.py:11-207 on the HIP path.

Same schedule construction (make_schedule, :24-54), same sampling loop order and
noise consumption (one N(0, I) draw of x's shape per step, :201), same update
(p_sample_ddim, :188-207) -- the update itself is one HIP kernel.

With ``use_graph=True`` (default on a HIP device, when no per-step callbacks or guidance are
requested) the WHOLE S-step loop -- S x (UNet forward + DDIM update), plus
the copies of the logged intermediates -- is captured into one HIP graph per (batch shape,
S, eta, log_every_t) and replayed once per ``sample()`` call.  Everything the graph reads
lives in buffers owned by its cache entry (x_T, the conditioning, the per-step noise table,
the timestep rows), so a later call with other inputs copies them in and replays; the
schedule coefficients are kernel arguments of the unrolled steps.  Loops longer than
``GRAPH_MAX_STEPS`` capture one step (coefficients and timestep looked up at a device step
index) and replay it S times.  The capture, the UNet's scope inside a loop (eps borrow, hoisted
K / V and FiLM rows), the noise sources and the loop / step choice come from
encdiff_amd/graph_loops.py; this file keeps the cache entries and the order of each loop's nodes.

Noise: with eta > 0 each captured step draws its N(0, I) row inside the graph (torch's
graph-safe Philox stream advances on every replay), so a loop holds one step's noise, not an
(S, *x.shape) table.  ``normals_sequence`` (the reference's kwarg, unused there) injects a
given table instead -- step i (in loop order, i = 0 .. S-1) adds sigma_i * normals_sequence[i]
-- which is how the eta > 0 trajectory is pinned against the reference's CPU noise stream.
At eta == 0 sigma is 0 for every step and no noise is drawn.  Either way the step noise is the
entry's graph_loops.NoiseRows ``z`` (the inpainting re-noise: ``mz``).

Inpainting (``mask`` + ``x0``) and ``quantize_x0`` run on the same captured paths: a masked step
re-noises the known region in front of the UNet (ops.masked_renoise, its N(0, I) row drawn inside
the graph, or taken from ``mask_normals_sequence`` -- S draws of x's shape in loop order, the
counterpart of ``normals_sequence``), a quantised step replaces pred_x0 by its nearest codebook
entry inside the update kernel (ops.ddim_step_quantized).  The mask and x0 live in buffers of the
cache entry like x_T and the conditioning.  The logged intermediates are the un-blended values
and the final sample is not blended, as in the reference's loop.

Before a replay the model's bf16 weight packs are refreshed if the parameters changed in
place since the capture (LatentDiffusion.refresh_hip_weights): a sampler captured outside
ema_scope() samples with the EMA weights inside it.

DDIMSamplerAttn (ddim.py:210-482) adds DDIM inversion on the same switches: see its docstring.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from encdiff_amd import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.encdiff.*)
from encdiff_amd.graph_loops import (NoiseRows, capture, kernel_mask, loop_or_step, noise_table, unet_loop,
                                     vq_codebook)
from ...modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps, noise_like

GRAPH_MAX_STEPS = 256  # longer loops replay a one-step graph (device step index)
# Capturing a whole S-step loop records S x ~300 kernel nodes (~4 s at S = 200), which only pays
# when the same (batch shape, S, eta) is sampled again: the first LOOP_GRAPH_AFTER calls of a
# loop replay the one-step graph (captured in milliseconds, ~1 % slower per step), later calls
# capture and replay the whole-loop graph.  A one-off call (the first log_images) then costs
# about its sampling time; repeated sampling (validation, the bench) runs the loop graph.
LOOP_GRAPH_AFTER = 1
# whole-loop graph: K / V of the conditioning and the FiLM rows of all steps computed once per loop
HOIST = os.environ.get("ENCDIFF_DDIM_HOIST", "1") != "0"


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", use_graph=True, **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.use_graph = use_graph
        self._graphs = {}
        self._seen = {}  # loop key -> sample() calls so far (LOOP_GRAPH_AFTER)
        # (S, eta) -> device coefficient / timestep tables.  Allocated once and kept: a
        # captured graph holds their addresses, so they are never rebound or freed.
        self._tables = {}

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor):
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps,
                                                  verbose=verbose)
        alphas_cumprod = self.model.alphas_cumprod
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps
        to_t = lambda x: x.clone().detach().to(torch.float32).to(self.model.device)  # noqa: E731
        self.register_buffer("betas", to_t(self.model.betas))
        self.register_buffer("alphas_cumprod", to_t(alphas_cumprod))
        self.register_buffer("alphas_cumprod_prev", to_t(self.model.alphas_cumprod_prev))
        ac = alphas_cumprod.cpu()
        self.register_buffer("sqrt_alphas_cumprod", to_t(torch.sqrt(ac)))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", to_t(torch.sqrt(1. - ac)))
        sig, a, ap, an = make_ddim_sampling_parameters(ac, self.ddim_timesteps, ddim_eta, verbose=verbose)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev, self.ddim_alphas_next = sig, a, ap, an
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - a)
        self.ddim_eta = ddim_eta
        key = (ddim_discretize, int(ddim_num_steps), float(ddim_eta))
        tab = self._tables.get(key)
        if tab is None:
            # coef[index] = (a_t, a_prev, sigma, sqrt(1 - a_t)); ts[index]
            coef = np.stack([a, ap, sig, self.ddim_sqrt_one_minus_alphas], axis=1).astype(np.float32)
            tab = self._tables[key] = (torch.tensor(coef, device=self.model.device),
                                       torch.tensor(np.asarray(self.ddim_timesteps, dtype=np.int64),
                                                    device=self.model.device))
        self._coef, self._ts = tab
        self._sched_key = key

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1.,
               noise_dropout=0., score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None,
               log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None,
               mask_normals_sequence=None, **kwargs):
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, temperature=temperature,
                                  noise_dropout=noise_dropout, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning,
                                  normals_sequence=normals_sequence, mask_normals_sequence=mask_normals_sequence)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, normals_sequence=None,
                      mask_normals_sequence=None):
        device = self.model.betas.device
        b = shape[0]
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float().contiguous()
        if ddim_use_original_steps:
            raise NotImplementedError("ddim_use_original_steps is not used by EncDiff")
        if timesteps is not None:
            end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            steps = self.ddim_timesteps[:end]
        else:
            steps = self.ddim_timesteps
        total = steps.shape[0]
        if normals_sequence is not None:
            normals_sequence = noise_table(normals_sequence, total, img.shape, device)
        if mask_normals_sequence is not None:
            mask_normals_sequence = noise_table(mask_normals_sequence, total, img.shape, device,
                                                "mask_normals_sequence")
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        kmask = None  # the mask in the re-noise kernel's layout, (B, 1, H, W) or (B, C, H, W)
        if mask is not None:
            assert x0 is not None, "inpainting needs x0 with the mask"
            kmask = kernel_mask(mask, img)
        simple = (callback is None and img_callback is None and (mask is None or kmask is not None) and
                  (not quantize_denoised or vq_codebook(self.model, img) is not None) and
                  noise_dropout == 0. and score_corrector is None and temperature == 1. and
                  (unconditional_conditioning is None or unconditional_guidance_scale == 1.))
        if self.use_graph and simple and img.is_cuda and timesteps is None and isinstance(cond, torch.Tensor):
            extra = dict(mask=kmask, x0=x0, quant=bool(quantize_denoised), mask_normals=mask_normals_sequence)
            lk = (tuple(img.shape), total, self._sched_key, tuple(cond.shape), cond.dtype, log_every_t,
                  bool(normals_sequence is not None and self.ddim_eta),
                  None if kmask is None else (tuple(kmask.shape), mask_normals_sequence is not None),
                  bool(quantize_denoised))
            run = self._loop_graph if self._path(lk, total) == "loop" else self._step_graph
            return run(cond, img, total, log_every_t, intermediates, normals_sequence, **extra)
        for i, step in enumerate(np.flip(steps)):
            index = total - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:
                mz = None if mask_normals_sequence is None else mask_normals_sequence[i]
                if kmask is not None and img.is_cuda:  # the captured loops' kernel
                    img = img.clone()  # the caller's x_T / a logged (un-blended) intermediate stays as it is
                    ops.masked_renoise(img, x0.float().contiguous(), torch.randn_like(img) if mz is None else mz,
                                       kmask, ts, self.model.sqrt_alphas_cumprod,
                                       self.model.sqrt_one_minus_alphas_cumprod)
                else:
                    img = self.model.q_sample(x0, ts, noise=mz) * mask + (1. - mask) * img
            img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, quantize_denoised=quantize_denoised,
                                              temperature=temperature, noise_dropout=noise_dropout,
                                              score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                              unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning,
                                              noise=None if normals_sequence is None else normals_sequence[i])
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total - 1:
                intermediates["x_inter"].append(img)
                intermediates["pred_x0"].append(pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, noise=None):
        b = x.shape[0]
        if unconditional_conditioning is None or unconditional_guidance_scale == 1.:
            e_t = self.model.apply_model(x, t, c)
        else:
            x_in, t_in = torch.cat([x] * 2), torch.cat([t] * 2)
            c_in = torch.cat([unconditional_conditioning, c])
            e_u, e_t = self.model.apply_model(x_in, t_in, c_in).chunk(2)
            e_t = e_u + unconditional_guidance_scale * (e_t - e_u)
        if score_corrector is not None:
            e_t = score_corrector.modify_score(self.model, e_t, x, t, c, **corrector_kwargs)
        a_t, a_prev = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])
        sigma, s1 = float(self.ddim_sigmas[index]), float(self.ddim_sqrt_one_minus_alphas[index])
        if noise is None:
            noise = noise_like(x.shape, x.device, repeat_noise)
        noise = noise * temperature
        if noise_dropout > 0.:
            noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        x = x.float().contiguous()
        e_t = e_t.float().contiguous()
        cb = vq_codebook(self.model, x) if quantize_denoised else None
        if cb is not None:
            x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
            ops.ddim_step_quantized(x, e_t, noise.float().contiguous(), (a_t, a_prev, sigma, s1), cb, x_prev, pred_x0)
            return x_prev, pred_x0
        if quantize_denoised:  # a codebook outside the kernel's limits: the torch quantiser
            pred_x0 = (x - s1 * e_t) / np.sqrt(a_t)
            pred_x0, _, _ = self.model.first_stage_model.quantize(pred_x0)
            x_prev = np.sqrt(a_prev) * pred_x0 + np.sqrt(1. - a_prev - sigma ** 2) * e_t + sigma * noise
            return x_prev, pred_x0
        return torch.ops.encdiff.ddim_step(x, e_t, noise, a_t, a_prev, sigma, s1)

    # ------------------------------------------------------------ captured loops
    def _path(self, key, total):
        """"loop" or "step" for this call of the loop ``key`` (graph_loops.loop_or_step)."""
        return loop_or_step(self._seen, key, total, LOOP_GRAPH_AFTER, GRAPH_MAX_STEPS)

    def _entry(self, kind, cond, img, total, log_every_t, normals, mask=None, x0=None, quant=False,
               mask_normals=None):
        """Cache entry (static input / output buffers) of a captured loop.  normals: the caller's
        normals_sequence table (None: the noise is drawn inside the graph).  mask / x0: inpainting
        (buffers of the entry, copied in per call; mask_normals: the re-noise table is injected
        too); quant: pred_x0 is quantised."""
        injected = bool(normals is not None and self.ddim_eta)
        mkey = None if mask is None else (tuple(mask.shape), mask_normals is not None)
        key = (kind, tuple(img.shape), total, self._sched_key, tuple(cond.shape), cond.dtype, log_every_t,
               injected, mkey, bool(quant))
        st = self._graphs.get(key)
        if st is None:
            dev = img.device
            logs = [i for i in range(total) if (total - i - 1) % log_every_t == 0 or i == 0]
            st = dict(key=key, x=torch.empty_like(img), x2=torch.empty_like(img), px0=torch.empty_like(img),
                      cond=torch.empty_like(cond), logs=logs,
                      log_x=torch.empty(len(logs), *img.shape, device=dev),
                      log_px0=torch.empty(len(logs), *img.shape, device=dev),
                      z=NoiseRows(total, img.shape, dev, injected, draw=bool(self.ddim_eta)), graph=None, mask=None,
                      codebook=vq_codebook(self.model, img) if quant else None)
            if mask is not None:
                st.update(mask=torch.empty_like(mask), x0=torch.empty_like(img),
                          mz=NoiseRows(total, img.shape, dev, mask_normals is not None))
            self._graphs[key] = st
        st["cond"].copy_(cond)
        st["x"].copy_(img)
        st["z"].fill(normals)
        if mask is not None:
            st["mask"].copy_(mask)
            st["x0"].copy_(x0)
            st["mz"].fill(mask_normals)
        return st

    def _refresh(self):
        f = getattr(self.model, "refresh_hip_weights", None)
        if f is not None:
            f()

    def _loop_graph(self, cond, img, total, log_every_t, intermediates, normals_sequence, **extra):
        """The whole loop as one HIP graph (unrolled: step i's coefficients and timestep are
        kernel arguments / a static timestep row)."""
        st = self._entry("loop", cond, img, total, log_every_t, normals_sequence, **extra)
        self._refresh()
        if st["graph"] is None:
            b = img.shape[0]
            steps = np.flip(self.ddim_timesteps)
            st["ts"] = torch.tensor(np.repeat(np.asarray(steps, dtype=np.int64)[:, None], b, axis=1), device=img.device)
            st["ts_col"] = st["ts"][:, 0].contiguous()  # one timestep per loop step (the FiLM table)
            st["graph"] = capture(lambda: self._loop_body(st, total), restore=st["x"], warm=True)
        st["graph"].replay()
        for j in range(len(st["logs"])):
            intermediates["x_inter"].append(st["log_x"][j].clone())
            intermediates["pred_x0"].append(st["log_px0"][j].clone())
        return st["out"].clone(), intermediates

    def _loop_body(self, st, total):
        x, xn = st["x"], st["x2"]
        logs = st["logs"]
        # ENCDIFF_DDIM_HOIST=0 recomputes K / V and the FiLM rows every step
        with unet_loop(self.model, st["ts_col"] if HOIST else None) as at:
            for i in range(total):
                index = total - i - 1
                at(i)
                if st["mask"] is not None:
                    self._renoise(st, x, st["ts"][i], st["mz"].row(i))
                e_t = self.model.apply_model(x, st["ts"][i], st["cond"])
                a_t, a_prev = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])
                sigma, s1 = float(self.ddim_sigmas[index]), float(self.ddim_sqrt_one_minus_alphas[index])
                z = st["z"].row(i)
                if st["codebook"] is not None:
                    ops.ddim_step_quantized(x, e_t.float().contiguous(), z, (a_t, a_prev, sigma, s1), st["codebook"],
                                            xn, st["px0"])
                else:
                    ops.ddim_step(x, e_t.float().contiguous(), z, a_t, a_prev, sigma, s1, xn, st["px0"])
                x, xn = xn, x
                if i in logs:
                    j = logs.index(i)
                    st["log_x"][j].copy_(x)
                    st["log_px0"][j].copy_(st["px0"])
        st["out"] = x

    def _renoise(self, st, x, t_row, z):
        """Kernel (a) in front of the UNet: the known region of x re-noised to the step's t."""
        ops.masked_renoise(x, st["x0"], z, st["mask"], t_row, self.model.sqrt_alphas_cumprod,
                           self.model.sqrt_one_minus_alphas_cumprod)

    def _step_graph(self, cond, img, total, log_every_t, intermediates, normals_sequence, **extra):
        """Loops longer than GRAPH_MAX_STEPS: one captured step (coefficients, timestep and
        noise row looked up at a device step index), replayed S times."""
        st = self._entry("step", cond, img, total, log_every_t, normals_sequence, **extra)
        self._refresh()
        b = img.shape[0]
        if st["graph"] is None:
            dev = img.device
            st.update(t=torch.empty(b, device=dev, dtype=torch.long), idx=torch.zeros(1, device=dev, dtype=torch.int32),
                      i=torch.zeros(1, device=dev, dtype=torch.long))
            st["idx"].fill_(total - 1)
            st["graph"] = capture(lambda: self._step_body(st), restore=st["x"], warm=True)
        st["idx"].fill_(total - 1)
        st["i"].zero_()
        for i in range(total):
            st["graph"].replay()
            if i in st["logs"]:
                intermediates["x_inter"].append(st["x"].clone())
                intermediates["pred_x0"].append(st["px0"].clone())
        return st["x"].clone(), intermediates

    def _step_body(self, st):
        idx = st["idx"]
        st["t"].copy_(self._ts.index_select(0, idx.long()).expand(st["t"].shape[0]))
        if st["mask"] is not None:  # the re-noise row is read (drawn) in front of the forward
            self._renoise(st, st["x"], st["t"], st["mz"].row_at(st["i"]))
        with unet_loop(self.model):
            e_t = self.model.apply_model(st["x"], st["t"], st["cond"])
        z = st["z"].row_at(st["i"])
        if st["z"].indexed or (st["mask"] is not None and st["mz"].indexed):
            st["i"].add_(1)  # the device counter of the injected tables
        if st["codebook"] is not None:
            ops.ddim_step_quantized(st["x"], e_t.float().contiguous(), z, self._coef, st["codebook"], st["x2"],
                                    st["px0"], index=idx, advance=True)
        else:
            ops.ddim_step_indexed(st["x"], e_t.float().contiguous(), z, self._coef, idx, st["x2"], st["px0"],
                                  advance=True)
        st["x"].copy_(st["x2"])


class DDIMSamplerAttn(DDIMSampler):
    """Mirror of ldm/models/diffusion/ddim.py:210-482: DDIMSampler's sampling with the
    ``return_context`` kwarg and the 'context' intermediates key, plus DDIM inversion
    (ddim_inversion / ddim_loop / next_step): the deterministic (eta = 0) DDIM update walked
    upwards in t, x_0 -> x_T, one UNet forward and one ops.ddim_invert_step launch per step.

    ``return_context=True`` is refused: the reference's UNetModel.forward swallows the kwarg
    (openaimodel_enc.py:712) and returns the eps tensor, so the reference's ``out[0]`` / ``out[1]``
    are batch rows of eps, not (eps, context) -- there is no context to mirror.

    The inversion loop runs on DDIMSampler's switches: eager (``use_graph=False``: host-scalar
    coefficients), a one-step graph (timestep row, coefficient row {a_t, a_next} and step index
    read on the device; the launch walks the index up; replayed S times) and, from the
    LOOP_GRAPH_AFTER-th call of a shape on and up to GRAPH_MAX_STEPS steps, the whole loop as one
    graph: step i reads slot i and writes slot i + 1 of a trajectory buffer (S + 1, B, C, H, W) of
    the cache entry, K / V of the conditioning and the FiLM rows of the S ascending timesteps
    computed once (HOIST).  Cache entries are keyed "inv_loop" / "inv_step", apart from the sampling
    graphs' "loop" / "step".  Every returned latent is a clone."""

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__(model, schedule=schedule, **kwargs)
        self._inv_tables = {}  # schedule key -> device table [S][2] = {a_t, a_next}, kept like _tables

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)
        tab = self._inv_tables.get(self._sched_key)
        if tab is None:
            coef = np.stack([self.ddim_alphas, self.ddim_alphas_next], axis=1).astype(np.float32)
            tab = self._inv_tables[self._sched_key] = torch.tensor(coef, device=self.model.device)
        self._inv_coef = tab

    @staticmethod
    def _no_context(return_context):
        if return_context:
            raise NotImplementedError(
                "return_context=True has nothing to mirror: the reference's UNetModel.forward swallows the "
                "kwarg (openaimodel_enc.py:712) and returns the eps tensor, so out[0] / out[1] in its "
                "DDIMSamplerAttn are batch rows of eps, not (eps, context)")

    # ------------------------------------------------------------ sampling: DDIMSampler's paths
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1.,
               noise_dropout=0., score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None,
               log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None,
               return_context=False, mask_normals_sequence=None, **kwargs):
        self._no_context(return_context)
        return super().sample(S, batch_size, shape, conditioning=conditioning, callback=callback,
                              normals_sequence=normals_sequence, img_callback=img_callback, quantize_x0=quantize_x0,
                              eta=eta, mask=mask, x0=x0, temperature=temperature, noise_dropout=noise_dropout,
                              score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, verbose=verbose,
                              x_T=x_T, log_every_t=log_every_t,
                              unconditional_guidance_scale=unconditional_guidance_scale,
                              unconditional_conditioning=unconditional_conditioning,
                              mask_normals_sequence=mask_normals_sequence, **kwargs)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, return_context=False,
                      normals_sequence=None, mask_normals_sequence=None):
        self._no_context(return_context)
        img, intermediates = super().ddim_sampling(
            cond, shape, x_T=x_T, ddim_use_original_steps=ddim_use_original_steps, callback=callback,
            timesteps=timesteps, quantize_denoised=quantize_denoised, mask=mask, x0=x0, img_callback=img_callback,
            log_every_t=log_every_t, temperature=temperature, noise_dropout=noise_dropout,
            score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
            unconditional_guidance_scale=unconditional_guidance_scale,
            unconditional_conditioning=unconditional_conditioning, normals_sequence=normals_sequence,
            mask_normals_sequence=mask_normals_sequence)
        intermediates["context"] = []
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, return_context=False,
                      noise=None):
        self._no_context(return_context)
        return super().p_sample_ddim(x, c, t, index, repeat_noise=repeat_noise, use_original_steps=use_original_steps,
                                     quantize_denoised=quantize_denoised, temperature=temperature,
                                     noise_dropout=noise_dropout, score_corrector=score_corrector,
                                     corrector_kwargs=corrector_kwargs,
                                     unconditional_guidance_scale=unconditional_guidance_scale,
                                     unconditional_conditioning=unconditional_conditioning, noise=noise)

    # ------------------------------------------------------------ inversion
    @torch.no_grad()
    def ddim_inversion(self, latent, cond, timesteps, ddim_use_original_steps=False, return_context=False):
        ddim_latents, intermediates = self.ddim_loop(latent, cond, timesteps, ddim_use_original_steps, return_context)
        return ddim_latents[-1], intermediates

    @torch.no_grad()
    def ddim_loop(self, latent, cond, timesteps, ddim_use_original_steps=False, return_context=False):
        """ddim.py:434-467: S = ``timesteps`` inversion steps in ascending order of ddim_timesteps;
        loop step i evaluates the model at t = ddim_timesteps[i] and applies next_step with
        a_t = ddim_alphas[i], a_next = ddim_alphas_next[i].  Returns (all_latent, {"context": []}),
        all_latent = [latent itself, then the S latents after each step]."""
        self._no_context(return_context)
        if ddim_use_original_steps:
            raise NotImplementedError("ddim_use_original_steps is not used by EncDiff")
        all_latent = [latent]
        self.make_schedule(ddim_num_steps=timesteps, ddim_eta=0., verbose=False)
        steps = self.ddim_timesteps
        total = steps.shape[0]
        intermediates = {"context": []}
        x = latent.clone().detach()
        if self.use_graph and x.is_cuda and isinstance(cond, torch.Tensor):
            x = x.float().contiguous()
            lk = ("inv", tuple(x.shape), total, self._sched_key, tuple(cond.shape), cond.dtype)
            run = self._inv_loop_graph if self._path(lk, total) == "loop" else self._inv_step_graph
            return all_latent + run(cond, x, total), intermediates
        b = x.shape[0]
        for i, step in enumerate(steps):
            ts = torch.full((b,), int(step), device=x.device, dtype=torch.long)
            e_t = self.model.apply_model(x, ts, cond)
            if x.is_cuda:
                x = x.float().contiguous()
                x_next = torch.empty_like(x)
                ops.ddim_invert_step(x, e_t.float().contiguous(), self._inv_row(i), x_next)
                x = x_next
            else:
                x = self.next_step(e_t, i, x, ddim_use_original_steps)
            all_latent.append(x)
        return all_latent, intermediates

    def next_step(self, model_output, index, sample, use_original_steps):
        """ddim.py:469-482, the reference's torch expression (any device; the captured and the eager
        HIP loops run ops.ddim_invert_step instead)."""
        b, device = model_output.shape[0], model_output.device
        alphas = self.model.alphas_cumprod if use_original_steps else self.ddim_alphas
        alphas_next = self.model.alphas_cumprod_next if use_original_steps else self.ddim_alphas_next
        a_t = torch.full((b, 1, 1, 1), float(alphas[index]), device=device)
        a_next = torch.full((b, 1, 1, 1), float(alphas_next[index]), device=device)
        b_t = 1 - a_t
        next_original_sample = (sample - b_t ** 0.5 * model_output) / a_t ** 0.5
        next_sample_direction = (1 - a_next) ** 0.5 * model_output
        return a_next ** 0.5 * next_original_sample + next_sample_direction

    def _inv_row(self, i):
        return float(self.ddim_alphas[i]), float(self.ddim_alphas_next[i])

    def _inv_entry(self, kind, cond, x, total):
        key = (kind, tuple(x.shape), total, self._sched_key, tuple(cond.shape), cond.dtype)
        st = self._graphs.get(key)
        if st is None:
            # slot 0: the caller's latent; the one-step graph updates slot 0 in place
            slots = total + 1 if kind == "inv_loop" else 1
            st = self._graphs[key] = dict(key=key, traj=torch.empty(slots, *x.shape, device=x.device),
                                          cond=torch.empty_like(cond), graph=None)
        st["cond"].copy_(cond)
        st["traj"][0].copy_(x)
        return st

    def _inv_loop_graph(self, cond, x, total):
        """The whole inversion loop as one HIP graph: step i reads slot i and writes slot i + 1 of
        the entry's trajectory buffer (no copy nodes); coefficients are kernel arguments."""
        st = self._inv_entry("inv_loop", cond, x, total)
        self._refresh()
        if st["graph"] is None:
            ts = np.asarray(self.ddim_timesteps, dtype=np.int64)
            st["ts"] = torch.tensor(np.repeat(ts[:, None], x.shape[0], axis=1), device=x.device)
            st["ts_col"] = st["ts"][:, 0].contiguous()  # ascending: the FiLM table of the loop
            # no restore: slot 0 is only read
            st["graph"] = capture(lambda: self._inv_loop_body(st, total), warm=True)
        st["graph"].replay()
        return [st["traj"][k].clone() for k in range(1, total + 1)]

    def _inv_loop_body(self, st, total):
        traj = st["traj"]
        with unet_loop(self.model, st["ts_col"] if HOIST else None) as at:
            for i in range(total):
                at(i)
                e_t = self.model.apply_model(traj[i], st["ts"][i], st["cond"])
                ops.ddim_invert_step(traj[i], e_t.float().contiguous(), self._inv_row(i), traj[i + 1])

    def _inv_step_graph(self, cond, x, total):
        """One captured inversion step (timestep and coefficient row looked up at a device step
        index that the launch walks up), replayed S times."""
        st = self._inv_entry("inv_step", cond, x, total)
        self._refresh()
        if st["graph"] is None:
            dev = x.device
            st.update(t=torch.empty(x.shape[0], device=dev, dtype=torch.long),
                      idx=torch.zeros(1, device=dev, dtype=torch.int32))
            self._inv_step_body(st)  # warm-up at row 0
            st["traj"][0].copy_(x)
            st["graph"] = capture(lambda: self._inv_step_body(st))
        st["idx"].zero_()
        out = []
        for _ in range(total):
            st["graph"].replay()
            out.append(st["traj"][0].clone())
        return out

    def _inv_step_body(self, st):
        x, idx = st["traj"][0], st["idx"]
        st["t"].copy_(self._ts.index_select(0, idx.long()).expand(st["t"].shape[0]))
        with unet_loop(self.model):
            e_t = self.model.apply_model(x, st["t"], st["cond"])
        ops.ddim_invert_step(x, e_t.float().contiguous(), self._inv_coef, x, index=idx, advance=True)
