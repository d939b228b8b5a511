"""Generate tests/golden/sampling.npz by running the REFERENCE sampling loops on the CPU.

    python tools/gen_golden_sampling.py [--out DIR]

Reuses the shims and build_ldm of tools/gen_golden.py (recipe weights, Shapes3D config).  Data
only: inputs, the seed of the draws, and outputs.  B = 2, latent 3 x 16 x 16, `cond` and `xT`
taken from ddim.npz, x0 (the known latent of the inpainting runs) = p_losses.npz's x0[:2], mask =
the centre square of log_images (ddpm_enc.py:1563-1567).

    anc_samples, anc_inter      p_sample_loop(timesteps=10, log_every_t=3): the final sample and
                                the intermediates [x_T, i = 9, 6, 3, 0]
    prog_samples, prog_x0       progressive_denoising(start_T=10, log_every_t=3): the final sample
                                and the x0_partial list [i = 9, 6, 3, 0]
    mddim_samples_eta{0,1},     DDIM S = 10 (log_every_t = 100) with mask and x0: the final sample
    mddim_pred_x0_last_eta{..}  and the last logged pred_x0

Noise: every run starts with torch.manual_seed(SEED) and consumes one CPU torch.randn of x's
shape per reference draw, in the reference's call order:
  * ancestral loops: one draw per step (p_sample's noise_like, ddpm_enc.py:1304), t == 0 included
    -- draw k belongs to step i = timesteps - 1 - k;
  * masked DDIM: per step the re-noise first (q_sample's randn_like in the sampling loop of
    ddim.py), the step noise second (p_sample_ddim's noise_like) -- draw 2k is the re-noise of
    loop step k, draw 2k + 1 its step noise (drawn at eta == 0 too, where sigma is 0).
tests/test_gpu_sampling.py regenerates the stream in that order and injects it through
normals_sequence / mask_normals_sequence.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402

SEED = 1234
STEPS = 10
LOG_EVERY_T = 3


def centre_mask(n, h, w):
    mask = torch.ones(n, h, w)
    mask[:, h // 4:3 * h // 4, w // 4:3 * w // 4] = 0.
    return mask[:, None, ...]


def generate():
    G.install_shims()
    torch.set_num_threads(8)
    from ldm.models.diffusion.ddim import DDIMSampler
    DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    torch.Tensor.cuda = lambda self, *a, **k: self
    ldm = G.build_ldm(G.load_yaml_cfg())
    fx = np.load(os.path.join(G.OUT, 'ddim.npz'))
    cond, xT = torch.tensor(fx['cond']), torch.tensor(fx['xT'])
    x0 = torch.tensor(np.load(os.path.join(G.OUT, 'p_losses.npz'))['x0'][:2])
    mask = centre_mask(2, 16, 16)
    res = dict(cond=cond.numpy(), xT=xT.numpy(), x0=x0.numpy(), mask=mask.numpy(), seed=np.array(SEED),
               steps=np.array(STEPS), log_every_t=np.array(LOG_EVERY_T))
    with torch.no_grad():
        torch.manual_seed(SEED)
        out, inter = ldm.p_sample_loop(cond, (2, 3, 16, 16), return_intermediates=True, x_T=xT.clone(),
                                       verbose=False, timesteps=STEPS, log_every_t=LOG_EVERY_T)
        res['anc_samples'], res['anc_inter'] = out.numpy(), torch.stack(inter).numpy()
        torch.manual_seed(SEED)
        out, inter = ldm.progressive_denoising(cond, (2, 3, 16, 16), verbose=False, x_T=xT.clone(), start_T=STEPS,
                                               log_every_t=LOG_EVERY_T)
        res['prog_samples'], res['prog_x0'] = out.numpy(), torch.stack(inter).numpy()
        for eta in (0.0, 1.0):
            torch.manual_seed(SEED)
            out, inter = DDIMSampler(ldm).sample(STEPS, 2, (3, 16, 16), cond, eta=eta, verbose=False, x_T=xT.clone(),
                                                 mask=mask, x0=x0)
            res[f'mddim_samples_eta{int(eta)}'] = out.numpy()
            res[f'mddim_pred_x0_last_eta{int(eta)}'] = inter['pred_x0'][-1].numpy()
    return res


def main():
    out = G.OUT
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(out, exist_ok=True)
    res = generate()
    np.savez_compressed(os.path.join(out, 'sampling.npz'), **res)
    print('sampling.npz written to', out, {k: v.shape for k, v in res.items()})


if __name__ == '__main__':
    main()
