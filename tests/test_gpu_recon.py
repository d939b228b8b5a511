"""GPU tests of the fused SSIM + MSE kernel (csrc/recon.hip) and of the scores built on it
(encdiff_amd/metrics.py, LatentDiffusion.reconstruction_metrics), against
tests/golden/recon_small.npz (the reference's own calculate_ssim / calculate_mse,
tools/gen_golden_recon.py) and the float64 numpy restatement tests/recon_restate.py.

Bounds.  SSIM: 1e-10 absolute against the restatement; MSE: 1e-12 relative.  Both sides are
float64 sums over the same float32 inputs and weights, of at most 121 terms per moment and ch * h * w
(at most 24576 here) per mean; they differ in the order of the sums and in contraction, a few
hundred ulps of 1.1e-16 at the very most.  Against the reference's recorded float32 values: the
deviation the recorder measured for that case (the reference's own rounding) on top of that.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import recon_restate as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recon_small.npz")
F32, F64 = torch.float32, torch.float64
SHAPES = {"ref_layout": (2, 64, 64, 3), "nchw": (2, 3, 64, 64), "ragged": (3, 2, 17, 23), "pixel": (2, 5, 1, 1),
          "window": (1, 1, 11, 11), "tiles": (2, 1, 40, 70), "one_tile": (1, 3, 16, 16), "flat_wide": (5, 1, 5, 33)}
CONST = {"const_nchw": (4, 3, 64, 64), "const_ref": (4, 64, 64, 3)}
SSIM_TOL, MSE_RTOL = 1e-10, 1e-12


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def ops():
    from encdiff_amd import ops
    assert ops.SSIM_WINDOW == 11
    return ops


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def data(gold):
    """Per fixture case, once: the images in [-1, 1] (float32) and the restatement's (ssim, mse) of
    their (x + 1.) / 2. maps."""
    out = {}
    for c, shape in SHAPES.items():
        xa, xb = R.from_u8(gold[c + "_a"]), R.from_u8(gold[c + "_b"])
        assert xa.shape == shape
        a, b = R.premap(xa), R.premap(xb)
        out[c] = (xa, xb, R.ssim(a, b, gold["window"]), R.mse(a, b))
    return out


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().tobytes()


def run(ops, a, b, pre=(0., 1.)):
    """Two launches into garbage; the second repeats bitwise.  float64 numpy (ssim, mse)."""
    n = a.shape[0]
    outs = []
    for fill in (float("nan"), 7.0):
        s, m = torch.full((n,), fill, device="cuda", dtype=F64), torch.full((n,), -fill, device="cuda", dtype=F64)
        rs, rm = ops.ssim_mse(a, b, pre[0], pre[1], out_ssim=s, out_mse=m)
        assert rs is s and rm is m
        outs.append((s.cpu().numpy(), m.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), \
        "launches differ"
    return outs[0]


def close(ssim, mse, want_ssim, want_mse, what, extra_ssim=0.0, extra_mse=0.0):
    es = np.abs(ssim - want_ssim).max()
    em = (np.abs(mse - want_mse) / np.maximum(np.abs(want_mse), 1e-300)).max()
    print(f"{what}: ssim off by {es:.3e} (bound {SSIM_TOL + extra_ssim:.3e}), mse by {em:.3e} relative "
          f"(bound {MSE_RTOL:.0e}{' + ' + format(extra_mse, '.1e') + ' absolute' if extra_mse else ''})")
    assert es <= SSIM_TOL + extra_ssim
    assert (np.abs(mse - want_mse) <= MSE_RTOL * np.abs(want_mse) + extra_mse).all()


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", list(SHAPES))
def test_ssim_mse(ops, gold, data, case):
    """Every shape against the restatement, and against the reference's recorded float32 values
    within the deviation recorded for the case."""
    xa, xb, want_s, want_m = data[case]
    ssim, mse = run(ops, up(xa), up(xb), (1., 0.5))
    assert ssim.shape == (xa.shape[0],) and ssim.dtype == np.float64
    close(ssim, mse, want_s, want_m, f"{case} vs the restatement")
    close(ssim, mse, gold[case + "_ssim_ref"].astype(np.float64), gold[case + "_mse_ref"].astype(np.float64),
          f"{case} vs the reference", float(gold[case + "_d_ssim"]), float(gold[case + "_d_mse"]))


def test_default_window_is_the_fixtures(ops, gold, data):
    """window=None uploads metrics.ssim_window(); passing the fixture's window gives the same bits."""
    xa, xb, _, _ = data["ragged"]
    a, b = up(xa), up(xb)
    s0, m0 = ops.ssim_mse(a, b)
    s1, m1 = ops.ssim_mse(a, b, window=up(gold["window"]))
    assert bits(s0) == bits(s1) and bits(m0) == bits(m1)
    assert s0.dtype == F64 and s0.shape == (3,) and s0.is_cuda


@pytest.mark.parametrize("case", list(SHAPES))
def test_identical_inputs(ops, data, case):
    xa = up(data[case][0])
    ssim, mse = run(ops, xa, xa.clone(), (1., 0.5))
    assert np.abs(ssim - 1.0).max() <= 1e-12
    assert (mse == 0.0).all()


@pytest.mark.parametrize("case", list(CONST))
def test_constant_images(ops, gold, case):
    """Images 0.7 and 0.63 everywhere: the reference's float32 conv(a a) - mu^2 cancels (it is off
    by the recorded 2.9e-4 in nchw); the kernel follows the float64 restatement."""
    shape = CONST[case]
    va, vb = (float(v) for v in gold["const_values"])
    a, b = torch.full(shape, va, device="cuda"), torch.full(shape, vb, device="cuda")
    want_s = R.ssim(a.cpu().numpy(), b.cpu().numpy(), gold["window"])
    want_m = R.mse(a.cpu().numpy(), b.cpu().numpy())
    ssim, mse = run(ops, a, b)
    close(ssim, mse, want_s, want_m, f"{case} vs the restatement")
    close(ssim, mse, gold[case + "_ssim_ref"].astype(np.float64), gold[case + "_mse_ref"].astype(np.float64),
          f"{case} vs the reference", float(gold[case + "_d_ssim"]), float(gold[case + "_d_mse"]))
    if case == "const_nchw":
        assert np.abs(ssim - gold[case + "_ssim_ref"]).min() > 1e-4   # the reference's own error, not ours


@pytest.mark.parametrize("case", ["ref_layout", "ragged", "tiles", "flat_wide"])
def test_strided_inputs_bitwise(ops, data, case):
    """Permuted memory (channels last) and a sliced view with a column step of 2 and margins give
    bitwise the contiguous result: the kernel reads through the four strides."""
    xa, xb, _, _ = data[case]
    a, b = up(xa), up(xb)
    base = run(ops, a, b, (1., 0.5))
    n, ch, h, w = a.shape
    last = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert last.shape == a.shape and (last.stride() != a.stride() or ch == 1)
    big = torch.full((n + 1, ch, h + 3, 2 * w + 1), float("nan"), device="cuda")
    view = big[1:, :, 2:h + 2, 1:2 * w:2]
    view.copy_(b)
    assert view.shape == b.shape and view.stride(3) == 2 and not view.is_contiguous()
    got = run(ops, last, view, (1., 0.5))
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    got = run(ops, view, last, (1., 0.5))   # a and b swapped: each has strides of its own
    swapped = run(ops, b, a, (1., 0.5))
    assert got[0].tobytes() == swapped[0].tobytes() and got[1].tobytes() == swapped[1].tobytes()


@pytest.mark.parametrize("case", ["ref_layout", "nchw", "ragged"])
def test_premap_is_the_scripts(ops, data, case):
    """(pre_add, pre_mul) = (1, 0.5) on [-1, 1] data is bitwise torch's float32 (x + 1.) / 2. done
    beforehand and passed with the identity map (0, 1)."""
    xa, xb, _, _ = data[case]
    a, b = up(xa), up(xb)
    fused = run(ops, a, b, (1., 0.5))
    ha, hb = (torch.from_numpy(xa) + 1.) / 2., (torch.from_numpy(xb) + 1.) / 2.
    assert ha.dtype == F32 and np.array_equal(ha.numpy(), R.premap(xa))
    host = run(ops, ha.cuda(), hb.cuda(), (0., 1.))
    assert fused[0].tobytes() == host[0].tobytes() and fused[1].tobytes() == host[1].tobytes()
    # and the device's own float32 arithmetic agrees with the host's
    dev = run(ops, (a + 1.) / 2., (b + 1.) / 2.)
    assert fused[0].tobytes() == dev[0].tobytes() and fused[1].tobytes() == dev[1].tobytes()


def test_outputs_at_an_offset_and_workspace_canaries(ops, data):
    """Outputs written inside longer buffers leave both neighbours alone; the workspace is written up
    to the queried size and not past it."""
    from encdiff_amd import _lib as L
    for case in ("tiles", "ref_layout", "flat_wide"):
        xa, xb, want_s, want_m = data[case]
        a, b = up(xa), up(xb)
        n = a.shape[0]
        sbuf = torch.full((n + 5,), -3.25, device="cuda", dtype=F64)
        mbuf = torch.full((n + 5,), 9.5, device="cuda", dtype=F64)
        ops.ssim_mse(a, b, 1., 0.5, out_ssim=sbuf[2:2 + n], out_mse=mbuf[3:3 + n])
        s, m = sbuf.cpu().numpy(), mbuf.cpu().numpy()
        assert (s[:2] == -3.25).all() and (s[2 + n:] == -3.25).all() and (m[:3] == 9.5).all() and (m[3 + n:] == 9.5).all()
        close(s[2:2 + n], m[3:3 + n], want_s, want_m, f"{case} at an offset")
        nbytes = ops.ssim_mse_workspace_bytes(*a.shape)
        assert nbytes % 16 == 0 and nbytes >= 16 * n * a.shape[1]
        ws = torch.full((nbytes // 8 + 64,), float("nan"), device="cuda", dtype=F64)
        args = ops.recon_args(a, b, 1., 0.5)
        so, mo = torch.empty(n, device="cuda", dtype=F64), torch.empty(n, device="cuda", dtype=F64)
        args.window, args.partial, args.ssim, args.mse = (t.data_ptr() for t in (ops._recon_window(a.device), ws, so, mo))
        L.check(L.lib.encdiff_ssim_mse(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ssim_mse")
        w = ws.cpu().numpy()
        assert np.isnan(w[nbytes // 8:]).all(), "written past the queried workspace size"
        assert not np.isnan(w[:nbytes // 8]).any(), "a partial was left unwritten"
        assert so.cpu().numpy().tobytes() == s[2:2 + n].tobytes() and mo.cpu().numpy().tobytes() == m[3:3 + n].tobytes()


def test_op_under_graph_capture(ops, data):
    """The op captured into a graph replays on fresh input contents to the eager bits (no host read,
    allocation or memset inside the op), from garbage in the outputs."""
    from encdiff_amd.graph_loops import capture
    xa, xb, _, _ = data["tiles"]
    a, b = up(xa), up(xb)
    n = a.shape[0]
    s, m = torch.empty(n, device="cuda", dtype=F64), torch.empty(n, device="cuda", dtype=F64)

    def body():
        ops.ssim_mse(a, b, 1., 0.5, out_ssim=s, out_mse=m)

    body()
    torch.cuda.synchronize()
    graph = capture(body)
    g = torch.Generator(device="cuda").manual_seed(11)
    for _ in range(2):
        a.copy_(torch.rand(a.shape, device="cuda", generator=g) * 2 - 1)
        b.copy_((a + 0.1 * torch.randn(a.shape, device="cuda", generator=g)).clamp(-1, 1))
        eager = ops.ssim_mse(a, b, 1., 0.5)
        s.fill_(float("nan")), m.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert bits(s) == bits(eager[0]) and bits(m) == bits(eager[1])
        want = R.ssim(R.premap(a.cpu().numpy()), R.premap(b.cpu().numpy()), ops._recon_window(a.device).cpu().numpy())
        assert np.abs(s.cpu().numpy() - want).max() <= SSIM_TOL


# ------------------------------------------------------------------ metrics.py
def test_metrics_functions(M, gold, data):
    """metrics.ssim / metrics.mse are calculate_ssim / calculate_mse on the tensors as given;
    reconstruction_scores is the script's call on (x0 (B, H, W, C), x_recon (B, C, H, W)) in [-1, 1]."""
    xa, xb, want_s, want_m = data["ref_layout"]          # (2, 64, 64, 3): an x0 as the data gives it
    x0 = up(xa)
    x_recon = up(xb).permute(0, 3, 1, 2).contiguous()    # (2, 3, 64, 64) as the decoder gives it
    ssim, mse = M.reconstruction_scores(x0, x_recon)
    close(ssim.cpu().numpy(), mse.cpu().numpy(), want_s, want_m, "reconstruction_scores, reference layout")
    a, b = (x0 + 1.) / 2., (up(xb) + 1.) / 2.
    assert bits(M.ssim(a, b)) == bits(ssim) and bits(M.mse(a, b)) == bits(mse)
    # nchw: the textbook call scores other planes and gives another number
    s2, m2 = M.reconstruction_scores(x0, x_recon, layout="nchw")
    pa, pb = R.premap(xa.transpose(0, 3, 1, 2)), R.premap(xb.transpose(0, 3, 1, 2))
    close(s2.cpu().numpy(), m2.cpu().numpy(), R.ssim(pa, pb, gold["window"]), R.mse(pa, pb),
          "reconstruction_scores, nchw")
    assert np.abs(s2.cpu().numpy() - ssim.cpu().numpy()).min() > 1e-3
    assert np.abs(m2.cpu().numpy() - mse.cpu().numpy()).max() <= 1e-12   # the mean over all pixels either way


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def ldm():
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


def test_reconstruction_metrics(ldm, M):
    """12 images in batches of 8 (a short last batch), S = 2: the per-image values are the scores of
    the returned images, the headline numbers the mean of the two batch means, and the two layouts
    differ."""
    g = torch.Generator(device="cuda").manual_seed(5)
    pool = torch.randint(0, 256, (12, 64, 64, 3), device="cuda", dtype=torch.uint8, generator=g)
    was = ldm.training
    out = ldm.reconstruction_metrics(pool=pool, ddim_steps=2, batch_size=8, return_images=True)
    assert ldm.training == was
    assert out["n"] == 12 and sorted(out) == ["mse", "n", "per_image", "ssim", "x0", "x_recon"]
    x0, xr = out["x0"], out["x_recon"]
    assert x0.shape == (12, 64, 64, 3) and xr.shape == (12, 3, 64, 64) and x0.is_cuda and xr.dtype == F32
    # the inputs, in dataset order (the gather normalises as ToTensor / Normalize do: an ulp off x / 127.5 - 1)
    assert np.abs(x0.cpu().numpy() - R.from_u8(pool.cpu().numpy())).max() <= 2.5e-7
    per = out["per_image"]
    assert per["ssim"].shape == (12,) and per["ssim"].dtype == np.float64 and np.isfinite(per["ssim"]).all()
    a, b = (x0 + 1.) / 2., ((xr + 1.) / 2.).permute(0, 2, 3, 1)
    assert per["ssim"].tobytes() == bits(M.ssim(a, b)) and per["mse"].tobytes() == bits(M.mse(a, b))
    for k in ("ssim", "mse"):
        want = np.mean([per[k][:8].mean(), per[k][8:].mean()])
        assert out[k] == want and abs(out[k] - per[k].mean()) > 0   # a short batch weighs as a whole one
    # max_images, float images in, and the other layout (the graphs of both batch sizes are reused)
    imgs = x0.clone()
    other = ldm.reconstruction_metrics(images=imgs, ddim_steps=2, batch_size=8, layout="nchw", return_images=True)
    assert other["n"] == 12 and torch.equal(other["x0"], x0)
    s2, m2 = M.reconstruction_scores(other["x0"], other["x_recon"], layout="nchw")
    assert other["per_image"]["ssim"].tobytes() == bits(s2) and other["per_image"]["mse"].tobytes() == bits(m2)
    s1, _ = M.reconstruction_scores(other["x0"], other["x_recon"], layout="reference")
    assert np.abs(s1.cpu().numpy() - other["per_image"]["ssim"]).max() > 1e-6, "the layouts gave the same SSIM"
    few = ldm.reconstruction_metrics(pool=pool, ddim_steps=2, batch_size=8, max_images=4)
    assert few["n"] == 4 and sorted(few) == ["mse", "n", "per_image", "ssim"] and few["ssim"] == few["per_image"]["ssim"].mean()
