"""Generate tests/golden/ddim_inversion.npz by running the REFERENCE DDIM inversion on the CPU.

    python tools/gen_golden_inversion.py [--out DIR]

Reuses the shims and build_ldm of tools/gen_golden.py (recipe weights, Shapes3D config).  Data
only: inputs and outputs.  B = 2, S = 10, latent 3 x 16 x 16, `cond` taken from ddim.npz, x0 (the
latent that is inverted) = p_losses.npz's x0[:2].  Inversion draws no noise.

    all_latent        (11, 2, 3, 16, 16)  DDIMSamplerAttn.ddim_loop(x0, cond, 10) in fp32:
                                          [x0, then the latent after each of the 10 steps]
    eps               (10, 2, 3, 16, 16)  the UNet's output at each step of that loop (recorded by
                                          wrapping apply_model): eps[k] was evaluated on all_latent[k]
    ddim_timesteps    (10,)               the loop's timesteps, ascending
    all_latent_bf16   (11, 2, 3, 16, 16)  the same loop under torch.autocast('cpu', bfloat16)
    bf16_rel          (10,)               rel-L2(all_latent_bf16[k], all_latent[k]), k = 1 .. 10

The bf16 run is the yardstick of this loop's sensitivity: with the recipe weights the UNet is not a
smooth ODE and the loop amplifies rounding differences, so the reference's own bf16 realisation
drifts from its fp32 one (bf16_rel is printed).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402

STEPS = 10


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def generate():
    G.install_shims()
    torch.set_num_threads(8)
    from ldm.models.diffusion.ddim import DDIMSamplerAttn
    DDIMSamplerAttn.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    torch.Tensor.cuda = lambda self, *a, **k: self
    ldm = G.build_ldm(G.load_yaml_cfg())
    cond = torch.tensor(np.load(os.path.join(G.OUT, 'ddim.npz'))['cond'])[:2]
    x0 = torch.tensor(np.load(os.path.join(G.OUT, 'p_losses.npz'))['x0'][:2])
    res = dict(cond=cond.numpy(), x0=x0.numpy(), steps=np.array(STEPS))

    eps = []
    inner = ldm.apply_model

    def recording(*a, **k):
        out = inner(*a, **k)
        eps.append(out.detach().float().clone())
        return out

    with torch.no_grad():
        sampler = DDIMSamplerAttn(ldm)
        ldm.apply_model = recording
        try:
            lat, _ = sampler.ddim_loop(x0.clone(), cond, STEPS)
        finally:
            ldm.apply_model = inner
        assert len(lat) == STEPS + 1 and len(eps) == STEPS
        res['all_latent'] = torch.stack(lat).numpy()
        res['eps'] = torch.stack(eps).numpy()
        res['ddim_timesteps'] = np.asarray(sampler.ddim_timesteps, dtype=np.int64)
        with torch.autocast('cpu', dtype=torch.bfloat16):
            lat16, _ = DDIMSamplerAttn(ldm).ddim_loop(x0.clone(), cond, STEPS)
        lat16 = [v.float() for v in lat16]
        res['all_latent_bf16'] = torch.stack(lat16).numpy()
        res['bf16_rel'] = np.asarray([rel(lat16[k], lat[k]) for k in range(1, STEPS + 1)])
    return res


def main():
    out = G.OUT
    if '--out' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1]
    os.makedirs(out, exist_ok=True)
    res = generate()
    np.savez_compressed(os.path.join(out, 'ddim_inversion.npz'), **res)
    print('ddim_inversion.npz written to', out, {k: v.shape for k, v in res.items()})
    print('rel-L2 bf16 autocast vs fp32, latents 1 .. %d:' % STEPS, ' '.join('%.3e' % v for v in res['bf16_rel']))


if __name__ == '__main__':
    main()
