"""CPU tests of DDIM inversion (DDIMSamplerAttn, csrc/sampler.hip's inversion step): the class has
the reference's shape, its schedule is the fixture's, next_step on CPU tensors reproduces every
step of the reference's recorded loop, what the reference does not implement is refused, argument
errors of the entry point come back without a device, and tests/golden/ddim_inversion.npz
regenerates bit-exactly from its tool where the reference tree exists.

next_step bound: the fp32 rule of tests/elementwise_restate.py, |out - ref64| <= floor + 2^-22
|ref64| per element, where ref64 is the header's expression evaluated in fp64 on the recorded
(latent, eps) and the floor is 4 x the largest distance of the same expression evaluated in fp32
from fp64.  The fixture's next latent (the reference's own fp32 evaluation) is held to the same rule.
"""
import ast
import ctypes as C
import inspect
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from elementwise_restate import F32, F64, f32_excess, floor_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_SHAPE = 0, -1, -2
METHODS = ("__init__", "make_schedule", "sample", "ddim_sampling", "p_sample_ddim", "ddim_inversion", "ddim_loop",
           "next_step")


@pytest.fixture(scope="module")
def fx(golden_dir):
    f = np.load(os.path.join(golden_dir, "ddim_inversion.npz"))
    return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def sched_model():
    """The Shapes3D schedule alone (no UNet), on the CPU."""
    import encdiff_amd  # noqa: F401
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import DDPM
    p = model_config("shapes3d")["params"]

    class Sched(DDPM):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.v_posterior, self.parameterization = 0., "eps"
            self.register_schedule(beta_schedule="linear", timesteps=p["timesteps"], linear_start=p["linear_start"],
                                   linear_end=p["linear_end"])

    return Sched()


@pytest.fixture()
def sampler(sched_model):
    import encdiff_amd  # noqa: F401
    from ldm.models.diffusion.ddim import DDIMSamplerAttn
    s = DDIMSamplerAttn(sched_model)
    s.make_schedule(10, ddim_eta=0., verbose=False)
    return s


def test_class_shape():
    import encdiff_amd  # noqa: F401
    from ldm.models.diffusion.ddim import DDIMSampler, DDIMSamplerAttn
    import encdiff_amd.ldm.models.diffusion.ddim as D
    import encdiff_amd.ldm.models.diffusion.ddpm_enc as E
    assert DDIMSamplerAttn is D.DDIMSamplerAttn and issubclass(DDIMSamplerAttn, DDIMSampler)
    assert E.DDIMSamplerAttn is DDIMSamplerAttn
    for m in METHODS:
        assert callable(getattr(DDIMSamplerAttn, m)), m
    for m in ("ddim_attn_sampler", "sample_log_attn"):
        assert callable(getattr(E.LatentDiffusion, m)), m
    assert E.LatentDiffusion.log_images_inversion is False
    assert hasattr(torch.ops.encdiff, "ddim_invert_step")


def _ref_signatures(path, cls):
    """{method: ([(name, default or inspect.Parameter.empty)], has **kwargs)} of a class, from the
    source text (the reference module is not imported)."""
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    out = {}
    for f in node.body:
        if not isinstance(f, ast.FunctionDef):
            continue
        a = f.args
        assert not a.posonlyargs and not a.kwonlyargs and a.vararg is None
        names = [x.arg for x in a.args]
        defaults = [inspect.Parameter.empty] * (len(names) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
        out[f.name] = (list(zip(names, defaults)), a.kwarg is not None)
    return out


def test_signatures_match_reference():
    """Every parameter of the reference's methods, in its order and with its default, leads ours;
    what we add behind them (the injected-noise kwargs of this project's DDIMSampler) has a default."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_golden
    finally:
        sys.path.pop(0)
    src = os.path.join(gen_golden.REF, "ldm", "models", "diffusion", "ddim.py")
    if not os.path.isfile(src):
        pytest.skip("the reference tree is not on this machine")
    import encdiff_amd  # noqa: F401
    from ldm.models.diffusion.ddim import DDIMSamplerAttn
    ref = _ref_signatures(src, "DDIMSamplerAttn")
    for m in METHODS:
        want, want_kw = ref[m]
        ps = list(inspect.signature(getattr(DDIMSamplerAttn, m)).parameters.values())
        have_kw = bool(ps) and ps[-1].kind is inspect.Parameter.VAR_KEYWORD
        if have_kw:
            ps = ps[:-1]
        assert have_kw == want_kw, m
        got = [(p.name, p.default) for p in ps]
        assert got[:len(want)] == want, (m, got, want)
        for p in ps[len(want):]:
            assert p.default is not inspect.Parameter.empty and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, (m, p)


def test_schedule(sampler, sched_model, fx):
    assert np.array_equal(np.asarray(sampler.ddim_timesteps), fx["ddim_timesteps"])
    ac = sched_model.alphas_cumprod.numpy()
    ts = fx["ddim_timesteps"]
    assert np.array_equal(sampler.ddim_alphas.astype(np.float32), ac[ts])
    for i in range(9):
        assert np.float32(sampler.ddim_alphas_next[i]) == ac[ts[i + 1]], i
    assert np.float32(sampler.ddim_alphas_next[9]) == ac[-1]
    # the device table of the captured step: {a_t, a_next} rows in loop order
    assert np.array_equal(sampler._inv_coef.numpy(), np.stack([ac[ts], np.append(ac[ts[1:]], ac[-1])], axis=1))


def invert_ref(x, e, a_t, a_next, dtype):
    """include/encdiff_hip.h, encdiff_ddim_invert_step: (x_out, x0); a_t, a_next fp32 values."""
    a, an = torch.tensor(a_t, dtype=F32).to(dtype), torch.tensor(a_next, dtype=F32).to(dtype)
    x, e = x.to(dtype), e.to(dtype)
    x0 = (x - (1 - a).sqrt() * e) / a.sqrt()
    return an.sqrt() * x0 + (1 - an).sqrt() * e, x0


def test_next_step_reproduces_the_recorded_loop(sampler, fx):
    lat, eps = torch.tensor(fx["all_latent"]), torch.tensor(fx["eps"])
    for k in range(10):
        a_t, a_next = float(sampler.ddim_alphas[k]), float(sampler.ddim_alphas_next[k])
        ref = invert_ref(lat[k], eps[k], a_t, a_next, F64)[0]
        floor = floor_of(invert_ref(lat[k], eps[k], a_t, a_next, F32)[0], ref)
        out = sampler.next_step(eps[k], k, lat[k], False)
        assert out.dtype == F32 and out.shape == lat[k].shape
        for what, v in (("next_step", out), ("fixture", lat[k + 1])):
            ex, i, worst = f32_excess(v, ref, floor)
            print(f"{what} k={k}: worst |err| {worst:.3e}, floor {floor:.3e}, excess {ex:.3e}")
            assert ex <= 0, (what, k, ex, i)


def test_refusals(sampler):
    x = torch.zeros(2, 3, 16, 16)
    cond = torch.zeros(2, 320)
    for call in (lambda: sampler.ddim_loop(x, cond, 10, return_context=True),
                 lambda: sampler.ddim_inversion(x, cond, 10, return_context=True),
                 lambda: sampler.sample(10, 2, (3, 16, 16), cond, verbose=False, x_T=x, return_context=True),
                 lambda: sampler.ddim_sampling(cond, (2, 3, 16, 16), x_T=x, return_context=True),
                 lambda: sampler.p_sample_ddim(x, cond, torch.zeros(2, dtype=torch.long), 0, return_context=True)):
        with pytest.raises(NotImplementedError, match="openaimodel_enc.py:712"):
            call()
    for call in (lambda: sampler.ddim_loop(x, cond, 10, ddim_use_original_steps=True),
                 lambda: sampler.ddim_inversion(x, cond, 10, True),
                 lambda: sampler.ddim_sampling(cond, (2, 3, 16, 16), x_T=x, ddim_use_original_steps=True)):
        with pytest.raises(NotImplementedError, match="ddim_use_original_steps"):
            call()


def _args(L, **kw):
    """A well-formed argument block over fake (never dereferenced) device addresses."""
    base = 1 << 32
    a = L.SamplerStepArgs(batch=2, c=3, hw=25, x=base, e=base + 4096, x_out=base + 8192, coef=base + 12288,
                          index=base + 16384)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invert_step_argument_errors_without_a_device():
    import encdiff_amd._lib as L
    f = L.lib.encdiff_ddim_invert_step
    far = (1 << 32) + 20480
    assert f(None, None) == ERR_ARG
    for miss in ("x", "e", "x_out"):
        assert f(C.byref(_args(L, **{miss: None})), None) == ERR_ARG, miss
    for bad in (dict(noise=far), dict(codebook=far), dict(n_e=64), dict(codebook=far, n_e=64), dict(clamp=1),
                dict(idx_out=far)):
        assert f(C.byref(_args(L, **bad)), None) == ERR_ARG, bad
    assert f(C.byref(_args(L, coef=None)), None) == ERR_ARG            # index without coef
    assert f(C.byref(_args(L, index=None)), None) == ERR_ARG           # coef without index
    assert f(C.byref(_args(L, coef=None, index=None, advance=1)), None) == ERR_ARG
    for bad in (dict(batch=0), dict(c=0), dict(hw=0), dict(batch=-1), dict(batch=1 << 16, c=1 << 7, hw=1 << 8)):
        assert f(C.byref(_args(L, **bad)), None) == ERR_SHAPE, bad
        assert f(C.byref(_args(L, coef=None, index=None, **bad)), None) == ERR_SHAPE, bad


def test_inversion_fixture_regenerates(golden_dir):
    tool = os.path.join(REPO, "tools", "gen_golden_inversion.py")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import gen_golden
    finally:
        sys.path.pop(0)
    if not os.path.isdir(gen_golden.REF):
        pytest.skip("the reference tree is not on this machine")
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, tool, "--out", d], check=True, capture_output=True, timeout=300)
        new = np.load(os.path.join(d, "ddim_inversion.npz"))
        old = np.load(os.path.join(golden_dir, "ddim_inversion.npz"))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert old[k].dtype == new[k].dtype and np.array_equal(old[k], new[k]), k


def test_fixture_records_the_loops_bf16_sensitivity(fx):
    """The reference's bf16-autocast loop against its fp32 loop: 4.2e-3, 1.16e-2 and 3.84e-2 rel-L2 at
    latents 1, 5 and 10 (the last above the project's 3e-2 DDIM bound)."""
    a, b = fx["all_latent_bf16"].astype(np.float64), fx["all_latent"].astype(np.float64)
    assert np.array_equal(a[0], b[0])
    r = np.array([np.linalg.norm(a[k] - b[k]) / np.linalg.norm(b[k]) for k in range(1, 11)])
    assert np.allclose(r, fx["bf16_rel"], rtol=1e-9)
    assert abs(r[0] - 4.2e-3) < 1e-4 and abs(r[4] - 1.16e-2) < 1e-4 and abs(r[9] - 3.84e-2) < 1e-4, r
    assert fx["all_latent"].shape == (11, 2, 3, 16, 16) and fx["eps"].shape == (10, 2, 3, 16, 16)
