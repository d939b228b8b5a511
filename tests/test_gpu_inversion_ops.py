"""Per-element tests of the DDIM inversion step kernel (csrc/sampler.hip, encdiff_ddim_invert_step)
against a restatement written from include/encdiff_hip.h and evaluated in fp64.

fp32 rule of tests/elementwise_restate.py: |out - ref64| <= floor + 2^-22 |ref64| per element, the
floor 4 x the largest distance of the same restatement evaluated in torch fp32 from fp64.  The pair
property (an inversion step followed by the DDIM step with a_t and a_next exchanged returns x) is
held to the same rule with the composite restatement: no other number is introduced.
"""
import ctypes as C
import math

import pytest
import torch

from elementwise_restate import F32, F64, ddim_step, f32_excess, floor_of, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 5, 5),        # less than one block
          (5, 3, 9, 9),        # 1215 elements: ragged, more than one block
          (1, 3, 593, 593)]    # 1 054 947 elements > 4096 x 256: the grid-stride loop and its tail
ROWS = [(10, 0), (10, 9), (200, 117)]  # (S, row); (10, 9): a_next = alphas_cumprod[-1]
OK, ERR_ARG, ERR_SHAPE = 0, -1, -2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


@pytest.fixture(scope="module")
def tables():
    """{S: device table [S][2] = {a_t, a_next}} of the Shapes3D schedule, as DDIMSamplerAttn builds them."""
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.models.diffusion.ddim import DDIMSamplerAttn
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import DDPM
    p = model_config("shapes3d")["params"]

    class Sched(DDPM):  # the schedule alone: no UNet
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.v_posterior, self.parameterization = 0., "eps"
            self.register_schedule(beta_schedule="linear", timesteps=p["timesteps"], linear_start=p["linear_start"],
                                   linear_end=p["linear_end"])

    m = Sched().cuda()
    s = DDIMSamplerAttn(m)
    out = {}
    for S in (10, 200):
        s.make_schedule(S, ddim_eta=0., verbose=False)
        out[S] = s._inv_coef
        assert out[S].shape == (S, 2) and out[S].dtype == F32
    assert out[10][9, 1].item() == m.alphas_cumprod[-1].item()
    return out


def check_f32(out, ref_fn, what):
    """ref_fn(dtype) -> the restatement in that dtype."""
    ref = ref_fn(F64)
    floor = floor_of(ref_fn(F32), ref)
    ex, i, worst = f32_excess(out, ref, floor)
    print(f"{what}: worst |err| {worst:.3e}, floor {floor:.3e}, excess {ex:.3e} at {i}")
    assert ex <= 0, (what, ex, i)


def invert_ref(x, e, row, dtype):
    """(x_out, x0) of encdiff_ddim_invert_step from the header; row = the fp32 pair {a_t, a_next}."""
    a, an = row[0].to(dtype), row[1].to(dtype)
    x, e = x.to(dtype), e.to(dtype)
    x0 = (x - (1 - a).sqrt() * e) / a.sqrt()
    return an.sqrt() * x0 + (1 - an).sqrt() * e, x0


def inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("S,row", ROWS)
def test_invert_step(tables, shape, S, row):
    from encdiff_amd import ops
    tab = tables[S]
    x, e = inputs(shape, 100 * S + row + shape[0])
    idx = torch.tensor([row], device="cuda", dtype=torch.int32)
    xn, x0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    ops.ddim_invert_step(x, e, tab, xn, x0, index=idx, advance=False)
    assert idx.item() == row, "advance=0 leaves the index"
    check_f32(x0, lambda dt: invert_ref(x, e, tab[row], dt)[1], f"x0 {shape} S={S} row {row}")
    check_f32(xn, lambda dt: invert_ref(x, e, tab[row], dt)[0], f"x_out {shape} S={S} row {row}")
    # host scalars: the same bits as the device table
    xh, x0h = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    ops.ddim_invert_step(x, e, tuple(tab[row].tolist()), xh, x0h)
    assert same_bits(xh, xn) and same_bits(x0h, x0)
    # x0_out absent
    xo = torch.full_like(x, float("nan"))
    ops.ddim_invert_step(x, e, tab, xo, None, index=idx, advance=False)
    assert same_bits(xo, xn)
    # x_out may alias x
    xa = x.clone()
    ops.ddim_invert_step(xa, e, tab, xa, None, index=idx, advance=False)
    assert same_bits(xa, xn)
    xb, x0b = x.clone(), torch.full_like(x, float("nan"))
    ops.ddim_invert_step(xb, e, tuple(tab[row].tolist()), xb, x0b)
    assert same_bits(xb, xn) and same_bits(x0b, x0)


def test_invert_advance_walks_rows_upwards(tables):
    """advance moves the index 0 -> S over S launches and uses rows 0 .. S - 1 in that order."""
    from encdiff_amd import ops
    tab = tables[10]
    shape = SHAPES[1]
    g = torch.Generator().manual_seed(31)
    x = torch.randn(shape, generator=g).cuda()
    idx = torch.zeros(1, device="cuda", dtype=torch.int32)
    for row in range(10):
        e = torch.randn(shape, generator=g).cuda()
        xn = torch.empty_like(x)
        ops.ddim_invert_step(x, e, tab, xn, None, index=idx, advance=True)
        assert idx.item() == row + 1, "advance increments the index by exactly one"
        check_f32(xn, lambda dt: invert_ref(x, e, tab[row], dt)[0], f"chained launch at row {row}")
        x = xn
    assert idx.item() == 10
    idx.fill_(4)
    ops.ddim_invert_step(x, e, tab, torch.empty_like(x), None, index=idx, advance=False)
    assert idx.item() == 4


def test_torch_op(tables):
    x, e = inputs(SHAPES[1], 5)
    a_t, a_next = tables[10][3].tolist()
    xn, x0 = torch.ops.encdiff.ddim_invert_step(x, e, a_t, a_next)
    check_f32(xn, lambda dt: invert_ref(x, e, tables[10][3], dt)[0], "torch op x_out")
    check_f32(x0, lambda dt: invert_ref(x, e, tables[10][3], dt)[1], "torch op x0")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.encdiff.ddim_invert_step(x.cpu(), e.cpu(), a_t, a_next)


@pytest.mark.parametrize("S,row", ROWS)
def test_ddim_step_undoes_the_inversion_step(tables, S, row):
    """ddim_step(x', e, a_t = a_next, a_prev = a_t, sigma = 0, s1 = sqrt(1 - a_next)) on the inversion
    step's output x' returns x."""
    from encdiff_amd import ops
    tab = tables[S]
    shape = SHAPES[1]
    x, e = inputs(shape, 7 + row)
    a_t, a_next = tab[row].tolist()
    s1 = math.sqrt(1 - a_next)
    xn = torch.empty_like(x)
    ops.ddim_invert_step(x, e, (a_t, a_next), xn)
    back = torch.full_like(x, float("nan"))
    ops.ddim_step(xn, e, None, a_next, a_t, 0.0, s1, back)

    def composite(dt):
        return ddim_step(invert_ref(x, e, tab[row], dt)[0], e, None, a_next, a_t, 0.0, s1, dtype=dt)[0]

    print(f"S={S} row {row}: |composite fp64 - x| max {(composite(F64) - x.double()).abs().max().item():.3e}, "
          f"|kernels - x| max {(back.double() - x.double()).abs().max().item():.3e}")
    check_f32(back, composite, f"pair S={S} row {row}")


def _block(xt, et, out, **kw):
    import encdiff_amd._lib as L
    B, Cc, H, W = xt.shape
    a = L.SamplerStepArgs(batch=B, c=Cc, hw=H * W, x=xt.data_ptr(), e=et.data_ptr(), x_out=out.data_ptr())
    a.coef_host = (C.c_float * 5)(0.9, 0.8, 0.0, 0.0, 0.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refusals_launch_nothing(tables):
    import encdiff_amd._lib as L
    f = L.lib.encdiff_ddim_invert_step
    x, e = inputs(SHAPES[0], 3)
    out, x0 = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    idx = torch.tensor([2], device="cuda", dtype=torch.int32)
    other = torch.zeros(4096, device="cuda")
    ints = torch.zeros(4096, device="cuda", dtype=torch.int32)
    tab = tables[10]
    s = torch.cuda.current_stream().cuda_stream
    p, ti = other.data_ptr(), (tab.data_ptr(), idx.data_ptr())
    arg = [dict(x=None), dict(e=None), dict(x_out=None), dict(noise=p), dict(codebook=p), dict(n_e=64),
           dict(codebook=p, n_e=64), dict(clamp=1), dict(idx_out=ints.data_ptr()),
           dict(index=ti[1]), dict(coef=ti[0]), dict(advance=1),
           dict(coef=ti[0], index=ti[1], advance=1, noise=p)]
    shp = [dict(batch=0), dict(c=0), dict(hw=0), dict(hw=-25), dict(batch=1 << 16, c=1 << 7, hw=1 << 8),
           dict(batch=0, coef=ti[0], index=ti[1], advance=1)]
    for bad in arg:
        assert f(C.byref(_block(x, e, out, x0_out=x0.data_ptr(), **bad)), s) == ERR_ARG, bad
    for bad in shp:
        assert f(C.byref(_block(x, e, out, x0_out=x0.data_ptr(), **bad)), s) == ERR_SHAPE, bad
    assert f(None, s) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (x0 == 7.0).all() and idx.item() == 2, "a refused call launched something"
    assert (other == 0).all() and (ints == 0).all()
    # the well-formed block is accepted
    assert f(C.byref(_block(x, e, out, x0_out=x0.data_ptr(), coef=ti[0], index=ti[1], advance=1)), s) == OK
    torch.cuda.synchronize()
    assert idx.item() == 3 and torch.isfinite(out).all() and not (out == 7.0).all()
