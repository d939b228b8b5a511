"""CPU tests of the sampling-step entry points (csrc/sampler.hip): the ctypes mirror of
EncdiffSamplerStepArgs has the C layout, argument errors come back without a device, the model's
ancestral coefficient table equals the reference's fp64 schedule formulas to fp32 rounding, and
tests/golden/sampling.npz regenerates bit-exactly from its tool where the reference tree exists."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "encdiff_hip.h")
OK, ERR_ARG, ERR_SHAPE = 0, -1, -2


def test_struct_layout_matches_c():
    import encdiff_amd._lib as L
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){",
             'printf("size %zu\\n", sizeof(EncdiffSamplerStepArgs));']
    for fname, _ in L.SamplerStepArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(EncdiffSamplerStepArgs, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        field, val = line.split()
        if field == "size":
            assert C.sizeof(L.SamplerStepArgs) == int(val)
        else:
            assert getattr(L.SamplerStepArgs, field).offset == int(val), field
        seen += 1
    assert seen == len(L.SamplerStepArgs._fields_) + 1


def _args(L, **kw):
    """A well-formed argument block over fake (never dereferenced) device addresses."""
    base = 1 << 32
    a = L.SamplerStepArgs(batch=2, c=3, hw=25, x=base, e=base + 4096, x_out=base + 8192, coef=base + 12288,
                          index=base + 16384)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_step_argument_errors_without_a_device():
    import encdiff_amd._lib as L
    lib = L.lib
    for fn in (lib.encdiff_ancestral_step, lib.encdiff_ddim_step_quantized):
        assert fn(None, None) == ERR_ARG
    cb = dict(codebook=(1 << 32) + 20480, n_e=64)
    for miss in ("x", "e", "x_out"):
        assert lib.encdiff_ancestral_step(C.byref(_args(L, **{miss: None})), None) == ERR_ARG, miss
        assert lib.encdiff_ddim_step_quantized(C.byref(_args(L, **cb, **{miss: None})), None) == ERR_ARG, miss
    # the ancestral step reads t from the table row: the table and the index are required
    assert lib.encdiff_ancestral_step(C.byref(_args(L, coef=None, index=None)), None) == ERR_ARG
    # an index without its table (and the reverse), advance without an index
    assert lib.encdiff_ancestral_step(C.byref(_args(L, coef=None)), None) == ERR_ARG
    assert lib.encdiff_ddim_step_quantized(C.byref(_args(L, **cb, index=None)), None) == ERR_ARG
    assert lib.encdiff_ddim_step_quantized(C.byref(_args(L, **cb, coef=None, index=None, advance=1)), None) == ERR_ARG
    # the quantised DDIM step needs its codebook; indices need a lookup
    assert lib.encdiff_ddim_step_quantized(C.byref(_args(L)), None) == ERR_ARG
    assert lib.encdiff_ancestral_step(C.byref(_args(L, n_e=64)), None) == ERR_ARG
    assert lib.encdiff_ancestral_step(C.byref(_args(L, idx_out=(1 << 32) + 24576)), None) == ERR_ARG
    # shapes
    for bad in (dict(batch=0), dict(c=0), dict(hw=0), dict(batch=1 << 20, hw=1 << 10)):
        assert lib.encdiff_ancestral_step(C.byref(_args(L, **bad)), None) == ERR_SHAPE, bad
    for bad in (dict(c=9), dict(n_e=8193), dict(n_e=-1)):
        assert lib.encdiff_ddim_step_quantized(C.byref(_args(L, **{**cb, **bad})), None) == ERR_SHAPE, bad
        assert lib.encdiff_ancestral_step(C.byref(_args(L, **{**cb, **bad})), None) == ERR_SHAPE, bad


def test_renoise_argument_errors_without_a_device():
    import encdiff_amd._lib as L
    f = L.lib.encdiff_masked_renoise
    p = [(1 << 32) + 4096 * i for i in range(7)]  # img, x0, z, mask, t, sqrt_ac, sqrt_1mac

    def call(ptrs, mask_c=1, batch=2, c=3, hw=25):
        img, x0, z, mask, t, sa, s1a = ptrs
        return f(img, x0, z, mask, mask_c, t, sa, s1a, batch, c, hw, None)

    for i in range(7):
        q = list(p)
        q[i] = None
        assert call(q) == ERR_ARG, i
    assert call(p, mask_c=2) == ERR_SHAPE  # neither 1 nor c
    assert call(p, mask_c=0) == ERR_SHAPE
    for bad in (dict(batch=0), dict(c=0, mask_c=1), dict(hw=0), dict(batch=1 << 16, c=1 << 8, hw=1 << 8, mask_c=1)):
        assert call(p, **bad) == ERR_SHAPE, bad


def test_ancestral_table_matches_fp64_schedule():
    """Rows of LatentDiffusion.ancestral_table() against register_schedule's formulas
    (ddpm_enc.py:133-187) evaluated in fp64 on the Shapes3D schedule."""
    import encdiff_amd  # noqa: F401
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import DDPM
    from encdiff_amd.ldm.modules.diffusionmodules.util import make_beta_schedule

    from encdiff_amd.configs import model_config
    p = model_config("shapes3d")["params"]
    T, lo, hi = p["timesteps"], p["linear_start"], p["linear_end"]
    assert T == 1000

    class Sched(DDPM):  # the schedule alone: no UNet
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.v_posterior, self.parameterization = 0., "eps"
            self.register_schedule(beta_schedule="linear", timesteps=T, linear_start=lo, linear_end=hi)

    tab = Sched().ancestral_table()
    assert tab.shape == (1000, 5) and tab.dtype == torch.float32 and tab.is_contiguous()
    betas = np.asarray(make_beta_schedule("linear", T, linear_start=lo, linear_end=hi), dtype=np.float64)
    alphas = 1. - betas
    ac = np.cumprod(alphas)
    ac_prev = np.append(1., ac[:-1])
    pv = betas * (1. - ac_prev) / (1. - ac)
    want = np.stack([np.sqrt(1. / ac), np.sqrt(1. / ac - 1), betas * np.sqrt(ac_prev) / (1. - ac),
                     (1. - ac_prev) * np.sqrt(alphas) / (1. - ac), np.log(np.maximum(pv, 1e-20))], axis=1)
    assert np.array_equal(tab.numpy(), want.astype(np.float32))
    assert tab[0, 4].item() == np.float32(np.log(1e-20))  # the clipped row: t == 0 adds no noise anyway


def test_sampling_fixture_regenerates(golden_dir):
    tool = os.path.join(REPO, "tools", "gen_golden_sampling.py")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_golden
    finally:
        sys.path.pop(0)
    if not os.path.isdir(gen_golden.REF):
        pytest.skip("the reference tree is not on this machine")
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, tool, "--out", d], check=True, capture_output=True, timeout=300)
        new = np.load(os.path.join(d, "sampling.npz"))
        old = np.load(os.path.join(golden_dir, "sampling.npz"))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k
