"""Per-element tests of the sampling-step kernels (csrc/sampler.hip) against restatements written
from include/encdiff_hip.h and evaluated in fp64.

fp32 rule of tests/elementwise_restate.py: |out - ref64| <= floor + 2^-22 |ref64| per element, the
floor 4 x the largest distance of the same restatement evaluated in torch fp32 from fp64.
Codebook indices follow the convention of test_gpu_vq_decode.py: equal to the fp64 argmin of the
fp64 pred_x0 wherever the fp64 gap between the best and the second-best squared distance is
>= 1e-4 max(1, best); the excluded rows are at most 2 % of all.
"""
import math

import pytest
import torch

from elementwise_restate import F32, F64, f32_excess, floor_of, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 5, 5), (5, 3, 9, 9)]  # the second: 1215 elements, more than one block, ragged tail
T_ROWS = {3: [0, 999, 417], 5: [0, 999, 1, 500, 998]}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


@pytest.fixture(scope="module")
def sched():
    """The Shapes3D schedule buffers and the ancestral table, on the device."""
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import DDPM
    p = model_config("shapes3d")["params"]

    class Sched(DDPM):  # the schedule alone: no UNet
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.v_posterior, self.parameterization = 0., "eps"
            self.register_schedule(beta_schedule="linear", timesteps=p["timesteps"], linear_start=p["linear_start"],
                                   linear_end=p["linear_end"])

    s = Sched().cuda()
    assert s.ancestral_table().shape == (1000, 5)
    return s


def check_f32(out, ref_fn, what):
    """ref_fn(dtype) -> the restatement in that dtype."""
    ref = ref_fn(F64)
    floor = floor_of(ref_fn(F32), ref)
    ex, i, worst = f32_excess(out, ref, floor)
    print(f"{what}: worst |err| {worst:.3e}, floor {floor:.3e}, excess {ex:.3e} at {i}")
    assert ex <= 0, (what, ex, i)


# ------------------------------------------------------------------ masked re-noise
def renoise_ref(img, x0, z, mask, t, sa, s1a, dtype):
    a = sa.to(dtype)[t][:, None, None, None]
    s = s1a.to(dtype)[t][:, None, None, None]
    m = mask.to(dtype)
    return m * (a * x0.to(dtype) + s * z.to(dtype)) + (1 - m) * img.to(dtype)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mask_c", ["one", "all"])
@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_masked_renoise(sched, shape, mask_c, kind):
    from encdiff_amd import ops
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(B * 7 + (mask_c == "all"))
    img, x0, z = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    mshape = (B, 1 if mask_c == "one" else Cc, H, W)
    u = torch.rand(mshape, generator=g)
    mask = (u < 0.5).float() if kind == "binary" else torch.where(u < 0.3, torch.zeros(()), torch.where(
        u > 0.7, torch.ones(()), u))
    mask = mask.cuda()
    t = torch.tensor(T_ROWS[B], device="cuda")
    sa, s1a = sched.sqrt_alphas_cumprod, sched.sqrt_one_minus_alphas_cumprod
    out = img.clone()
    ops.masked_renoise(out, x0, z, mask, t, sa, s1a)
    q = torch.empty_like(img)
    ops.q_sample(x0, z, t, sa, s1a, q)
    full = mask.expand(shape)
    assert (full == 0).any() and (full == 1).any()
    assert same_bits(out[full == 0], img[full == 0]), "mask == 0 must leave img's bits"
    assert same_bits(out[full == 1], q[full == 1]), "mask == 1 must give the q_sample kernel's value"
    check_f32(out, lambda dt: renoise_ref(img, x0, z, mask, t, sa, s1a, dt), f"renoise {shape} {mask_c} {kind}")
    if kind == "fractional":
        assert ((full > 0) & (full < 1)).any()


# ------------------------------------------------------------------ ancestral step
def ancestral_ref(x, e, z, tab, row, clamp, dtype, code=None):
    """(x', x_recon) of encdiff_ancestral_step from the header; code: the quantised x_recon."""
    c0, c1, m1, m2, lv = [v.to(dtype) for v in tab[row]]
    xr = c0 * x.to(dtype) - c1 * e.to(dtype)
    if clamp:
        xr = xr.clamp(-1.0, 1.0)
    if code is not None:
        xr = code.to(dtype)
    mean = m1 * xr + m2 * x.to(dtype)
    if row != 0 and z is not None:
        mean = mean + torch.exp(0.5 * lv) * z.to(dtype)
    return mean, xr


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("row", [0, 1, 500, 999])
@pytest.mark.parametrize("clamp", [False, True])
def test_ancestral_step(sched, shape, row, clamp):
    from encdiff_amd import ops
    tab = sched.ancestral_table()
    g = torch.Generator().manual_seed(row + shape[0])
    x, e, z = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    idx = torch.tensor([row], device="cuda", dtype=torch.int32)
    xp, xr = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    ops.ancestral_step(x, e, z, tab, idx, xp, xr, clamp=clamp, advance=False)
    assert idx.item() == row
    raw = ancestral_ref(x, e, z, tab, row, False, F64)[1]
    assert (raw > 1).any() and (raw < -1).any() and (raw.abs() < 1).any(), "x_recon must straddle +-1"
    check_f32(xr, lambda dt: ancestral_ref(x, e, z, tab, row, clamp, dt)[1], f"x_recon row {row} clamp {clamp}")
    check_f32(xp, lambda dt: ancestral_ref(x, e, z, tab, row, clamp, dt)[0], f"x' row {row} clamp {clamp}")
    if clamp:
        assert xr.abs().max().item() <= 1.0 and (xr.abs() == 1.0).any()
    # x_out may alias x
    xa = x.clone()
    ops.ancestral_step(xa, e, z, tab, idx, xa, None, clamp=clamp, advance=False)
    assert same_bits(xa, xp)
    if row == 0:  # no noise at t == 0: the mean, bitwise, whatever z holds
        big, none = torch.empty_like(x), torch.empty_like(x)
        ops.ancestral_step(x, e, torch.full_like(x, 1e30), tab, idx, big, None, clamp=clamp, advance=False)
        ops.ancestral_step(x, e, None, tab, idx, none, None, clamp=clamp, advance=False)
        assert same_bits(big, xp) and same_bits(none, xp)
        check_f32(none, lambda dt: ancestral_ref(x, e, None, tab, 0, clamp, dt)[0], "mean at row 0")


def test_ancestral_advance_walks_rows(sched):
    from encdiff_amd import ops
    tab = sched.ancestral_table()
    shape = SHAPES[1]
    g = torch.Generator().manual_seed(21)
    x = torch.randn(shape, generator=g).cuda()
    idx = torch.tensor([2], device="cuda", dtype=torch.int32)
    for row in (2, 1, 0):
        e, z = (torch.randn(shape, generator=g).cuda() for _ in range(2))
        xp = torch.empty_like(x)
        ops.ancestral_step(x, e, z, tab, idx, xp, None, advance=True)
        assert idx.item() == row - 1, "advance decrements the index by exactly one"
        check_f32(xp, lambda dt: ancestral_ref(x, e, z, tab, row, False, dt)[0], f"chained launch at row {row}")
        x = xp
    assert idx.item() == -1


# ------------------------------------------------------------------ quantised steps
QUANT_CASES = [(2048, 3, 2, 5),     # 50 pixels: 64 lanes per pixel
               (2048, 3, 40, 16),   # 10240 pixels: the reduced split
               (3000, 4, 3, 7),     # two LDS chunks
               (37, 4, 3, 5)]       # fewer codes than lanes of a wave
# (a_t, a_prev, sigma): s1 = sqrt(1 - a_t)
COEFS = [(0.9, 0.95, 0.1), (0.05, 0.1, 0.2)]


def rows_of(z):
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])


def nchw_of(rows, like):
    B, Cc, H, W = like.shape
    return rows.view(B, H, W, Cc).permute(0, 3, 1, 2).contiguous()


def fp64_argmin_gap(p64, E):
    """Per pixel of p64 (NCHW fp64): the fp64 argmin over E, the best squared distance and the gap
    to the second best.  Chunked: the distance matrix of 10240 x 2048 x 3 doubles is 0.5 GB."""
    r = rows_of(p64)
    E64 = E.double()
    want, best, gap = [], [], []
    for s in range(0, r.shape[0], 2048):
        d = ((r[s:s + 2048, None, :] - E64[None]) ** 2).sum(-1)
        b2 = torch.topk(d, 2, dim=1, largest=False).values
        want.append(torch.argmin(d, dim=1))
        best.append(b2[:, 0])
        gap.append(b2[:, 1] - b2[:, 0])
    return torch.cat(want), torch.cat(best), torch.cat(gap)


def quant_inputs(case, seed):
    n_e, e_dim, B, H = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, e_dim, H, H, generator=g).cuda()
    e = torch.randn(B, e_dim, H, H, generator=g).cuda()
    E = torch.randn(n_e, e_dim, generator=g).cuda()
    z = torch.randn(B, e_dim, H, H, generator=g).cuda()
    return x, e, E, z


def f32v(v):
    return torch.tensor(v, dtype=F32)


def ddim_pred(x, e, a_t, dtype):
    a, s1 = f32v(a_t).to(dtype), f32v(math.sqrt(1 - a_t)).to(dtype)
    return (x.to(dtype) - s1 * e.to(dtype)) / a.sqrt()


def ddim_next(code, e, z, a_prev, sigma, dtype):
    ap, sg = f32v(a_prev).to(dtype), f32v(sigma).to(dtype)
    return ap.sqrt() * code.to(dtype) + (1.0 - ap - sg ** 2).sqrt() * e.to(dtype) + sg * z.to(dtype)


def check_quantised(tag, idx, px0, E, p64, keep_out):
    """Indices vs the fp64 argmin under the gap rule; pred_x0 bitwise the code of the index taken.
    Returns (kept-row mask NCHW, the code tensor NCHW of the kernel's indices)."""
    n = idx.numel()
    want, best, gap = fp64_argmin_gap(p64, E)
    keep = gap >= 1e-4 * best.clamp_min(1.0)
    for r in keep_out:
        keep[r] = False
    excluded = (~keep).sum().item()
    print(f"{tag}: {excluded} of {n} rows excluded ({100.0 * excluded / n:.2f} %)")
    assert excluded <= 0.02 * n + len(keep_out)
    assert (idx >= 0).all() and (idx < E.shape[0]).all()
    assert torch.equal(idx.long()[keep], want[keep])
    code = nchw_of(E[idx.long()], px0)
    assert same_bits(px0, code), "pred_x0 must be the codebook entry itself"
    km = nchw_of(keep[:, None].expand(-1, px0.shape[1]).contiguous(), px0)
    return km, code


@pytest.mark.parametrize("case", QUANT_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("coef", COEFS, ids=["a0.9", "a0.05"])
def test_ddim_step_quantized(case, coef):
    from encdiff_amd import ops
    a_t, a_prev, sigma = coef
    s1 = math.sqrt(1 - a_t)
    x, e, E, z = quant_inputs(case, QUANT_CASES.index(case))
    n = x.shape[0] * x.shape[2] * x.shape[3]
    idx = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    xp, px0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    ops.ddim_step_quantized(x, e, z, (a_t, a_prev, sigma, s1), E, xp, px0, idx=idx)
    km, code = check_quantised(f"ddim {case} a_t {a_t}", idx, px0, E, ddim_pred(x, e, a_t, F64), ())
    ref = lambda dt: ddim_next(code, e, z, a_prev, sigma, dt)[km]  # noqa: E731
    check_f32(xp[km], ref, f"ddim x' {case} a_t {a_t}")
    # the indexed form (device table, row 1 of 2) gives the same bits, and advances
    tab = torch.tensor([[0.5, 0.6, 0.0, math.sqrt(0.5)], [a_t, a_prev, sigma, s1]], device="cuda")
    row = torch.tensor([1], device="cuda", dtype=torch.int32)
    xi, pi = torch.empty_like(x), torch.empty_like(x)
    ops.ddim_step_quantized(x, e, z, tab, E, xi, pi, index=row, advance=True)  # no idx output
    assert row.item() == 0
    assert same_bits(xi, xp) and same_bits(pi, px0)
    # no noise: sigma z dropped
    xn = torch.empty_like(x)
    ops.ddim_step_quantized(x, e, None, (a_t, a_prev, sigma, s1), E, xn, None)
    check_f32(xn[km], lambda dt: ddim_next(code, e, torch.zeros_like(z), a_prev, sigma, dt)[km], "ddim x', no noise")


def synth_table(a_ts):
    """Rows 1.. of an ancestral table for the given a_t (row 0 unused: t == 0 adds no noise)."""
    rows = [[1.0, 0.0, 1.0, 0.0, 0.0]]
    for a in a_ts:
        rows.append([math.sqrt(1 / a), math.sqrt(1 / a - 1), 0.3, 0.7, -2.0])
    return torch.tensor(rows, dtype=F32).cuda()


@pytest.mark.parametrize("case", QUANT_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("ci", [0, 1], ids=["a0.9", "a0.05"])
def test_ancestral_step_quantized(case, ci):
    from encdiff_amd import ops
    tab = synth_table([c[0] for c in COEFS])
    row = ci + 1
    x, e, E, z = quant_inputs(case, QUANT_CASES.index(case))
    n = x.shape[0] * x.shape[2] * x.shape[3]
    idx = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    r = torch.tensor([row], device="cuda", dtype=torch.int32)
    xp, xr = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    ops.ancestral_step(x, e, z, tab, r, xp, xr, advance=False, codebook=E, idx=idx)
    km, code = check_quantised(f"ancestral {case} row {row}", idx, xr, E,
                               ancestral_ref(x, e, z, tab, row, False, F64)[1], ())
    check_f32(xp[km], lambda dt: ancestral_ref(x, e, z, tab, row, False, dt, code=code)[0][km],
              f"ancestral x' {case} row {row}")
    # clamp comes before the search (on the case with enough pixels for the excluded share to mean something)
    if n < 1000:
        return
    ic = torch.full_like(idx, -1)
    xc, xrc = torch.empty_like(x), torch.empty_like(x)
    ops.ancestral_step(x, e, z, tab, r, xc, xrc, clamp=True, advance=False, codebook=E, idx=ic)
    check_quantised(f"ancestral {case} row {row} clamp", ic, xrc, E,
                    ancestral_ref(x, e, z, tab, row, True, F64)[1], ())


@pytest.mark.parametrize("kind", ["ddim", "ancestral"])
def test_quantised_tie_goes_to_lowest_index(kind):
    """Codebook row 10 duplicated at row 2500 of the 3000-code case (the duplicate lies in the second
    LDS chunk) and one pixel's pred_x0 placed exactly on it: a_t = 0.25 makes 1 / sqrt(a_t) = 2
    exact, so with e = 0 and x = E[10] / 2 the pixel's pred_x0 is E[10] bitwise."""
    from encdiff_amd import ops
    case = QUANT_CASES[2]
    x, e, E, z = quant_inputs(case, 2)
    E[2500] = E[10]
    b, y, w = 1, 3, 4
    x[b, :, y, w] = E[10] / 2
    e[b, :, y, w] = 0
    H = case[3]
    pix = (b * H + y) * H + w
    idx = torch.full((x.shape[0] * H * H,), -1, device="cuda", dtype=torch.int32)
    xp, px0 = torch.empty_like(x), torch.empty_like(x)
    if kind == "ddim":
        ops.ddim_step_quantized(x, e, z, (0.25, 0.3, 0.1, math.sqrt(0.75)), E, xp, px0, idx=idx)
        p64 = ddim_pred(x, e, 0.25, F64)
    else:
        tab = synth_table([0.25])
        r = torch.tensor([1], device="cuda", dtype=torch.int32)
        ops.ancestral_step(x, e, z, tab, r, xp, px0, advance=False, codebook=E, idx=idx)
        p64 = ancestral_ref(x, e, z, tab, 1, False, F64)[1]
    assert torch.equal(rows_of(p64)[pix], E[10].double()), "the pixel is not exactly on the code"
    assert idx[pix].item() == 10
    check_quantised(f"tie {kind}", idx, px0, E, p64, (pix,))  # an exact tie: gap 0, checked above


def test_quantised_steps_reject_unsupported_shapes():
    from encdiff_amd import ops
    from encdiff_amd._lib import HipError
    coef = (0.9, 0.95, 0.1, math.sqrt(0.1))
    tab = synth_table([0.9])
    r = torch.tensor([1], device="cuda", dtype=torch.int32)
    for ch, n_e in ((9, 16), (3, 8193)):
        x = torch.randn(1, ch, 2, 2, device="cuda")
        E = torch.randn(n_e, ch, device="cuda")
        out = torch.full_like(x, 7.0)
        with pytest.raises(HipError, match="ENCDIFF_ERR_SHAPE"):
            ops.ddim_step_quantized(x, x, None, coef, E, out)
        with pytest.raises(HipError, match="ENCDIFF_ERR_SHAPE"):
            ops.ancestral_step(x, x, None, tab, r, out, advance=True, codebook=E)
        assert (out == 7.0).all() and r.item() == 1, "nothing was launched"
