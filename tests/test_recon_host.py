"""CPU tests of the host half of the reconstruction scores (encdiff_amd/metrics.py: ssim_window,
reconstruction_views and the refusals; ops.recon_args; the C-ABI's refusals, all before anything is
launched) and of the float64 numpy restatement the GPU tests lean on (tests/recon_restate.py),
against tests/golden/recon_small.npz: inputs and the output of the reference's own calculate_ssim,
create_window and calculate_mse, recorded by tools/gen_golden_recon.py.

Bound of the restatement against the reference: the deviation the recorder measured per case (the
reference's float32 rounding: at most 2.7e-7 on the noisy cases, 2.9e-4 on the constant nchw case
where its conv(a a) - mu^2 cancels) plus 1e-12 for the order of the float64 sums.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import recon_restate as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "encdiff_hip.h")
GOLD = os.path.join(REPO, "tests", "golden", "recon_small.npz")
OK, ERR_ARG, ERR_SHAPE = 0, -1, -2
SHAPES = {"ref_layout": (2, 64, 64, 3), "nchw": (2, 3, 64, 64), "ragged": (3, 2, 17, 23), "pixel": (2, 5, 1, 1),
          "window": (1, 1, 11, 11), "tiles": (2, 1, 40, 70), "one_tile": (1, 3, 16, 16), "flat_wide": (5, 1, 5, 33)}
CONST = {"const_nchw": (4, 3, 64, 64), "const_ref": (4, 64, 64, 3)}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


def case_images(gold, case):
    """float32 images in [0, 1] as the reference's functions got them."""
    if case in CONST:
        a, b = (np.full(tuple(gold[case + "_shape"]), v, np.float32) for v in gold["const_values"])
        return a, b
    return R.premap(R.from_u8(gold[case + "_a"])), R.premap(R.from_u8(gold[case + "_b"]))


def test_fixture_conditions(gold):
    assert gold["cases"].tolist() == list(SHAPES) and gold["const_cases"].tolist() == list(CONST)
    for case, shape in SHAPES.items():
        assert gold[case + "_a"].shape == shape and gold[case + "_a"].dtype == np.uint8
        assert gold[case + "_ssim_ref"].dtype == np.float32 and gold[case + "_ssim_f64"].dtype == np.float64
        assert gold[case + "_d_ssim"] <= 1e-6 and gold[case + "_d_mse"] <= 1e-6
    for case, shape in CONST.items():
        assert tuple(gold[case + "_shape"]) == shape
    assert gold["const_values"].tolist() == [np.float32(0.7), np.float32(0.63)]
    # the record of the reference's cancellation: large in nchw, absent where the plane is 64 x 3
    assert 1e-4 < gold["const_nchw_d_ssim"] < 1e-3 and gold["const_ref_d_ssim"] < 1e-6
    assert os.path.getsize(GOLD) <= 256 * 1024


def test_window_bitwise(gold, M):
    w = M.ssim_window()
    assert tuple(w.shape) == (11, 11) and w.is_contiguous() and str(w.dtype) == "torch.float32"
    assert w.numpy().tobytes() == gold["window"].tobytes()
    assert M.SSIM_WINDOW == 11
    total = float(gold["window"].astype(np.float64).sum())
    assert abs(total - 0.99999993) < 1e-8 and total != 1.0   # kept as the reference has it, not renormalised
    # not separable: the float32 outer product of the float32 row sums is another matrix
    g = gold["window"].sum(axis=1, dtype=np.float32)
    assert not np.array_equal(np.outer(g, g).astype(np.float32), gold["window"])


@pytest.mark.parametrize("case", list(SHAPES) + list(CONST))
def test_restatement_reproduces_reference(gold, case):
    a, b = case_images(gold, case)
    ssim, mse = R.ssim(a, b, gold["window"]), R.mse(a, b)
    assert ssim.dtype == np.float64 and ssim.shape == (a.shape[0],)
    es = np.abs(ssim - gold[case + "_ssim_ref"].astype(np.float64)).max()
    em = np.abs(mse - gold[case + "_mse_ref"].astype(np.float64)).max()
    print(f"{case}: restatement vs reference: ssim {es:.3e} (recorded d {float(gold[case + '_d_ssim']):.3e}), "
          f"mse {em:.3e} (recorded d {float(gold[case + '_d_mse']):.3e})")
    assert es <= gold[case + "_d_ssim"] + 1e-12 and em <= gold[case + "_d_mse"] + 1e-12
    assert np.abs(ssim - gold[case + "_ssim_f64"]).max() <= 1e-12
    assert np.abs(mse - gold[case + "_mse_f64"]).max() <= 1e-12 * gold[case + "_mse_f64"].max()


def test_restatement_by_hand(gold):
    """A single pixel: the window's only in-plane tap is its centre weight c, so mu = c a, the second
    moments c a^2, and the map follows from the formula in plain Python floats."""
    c = float(gold["window"][5, 5])
    a, b = np.float32(0.75), np.float32(0.25)
    m1, m2 = c * 0.75, c * 0.25
    s1, s2, s12 = c * 0.75 ** 2 - m1 * m1, c * 0.25 ** 2 - m2 * m2, c * 0.75 * 0.25 - m1 * m2
    want = ((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s1 + s2 + 9e-4))
    got = R.ssim(np.full((1, 1, 1, 1), a), np.full((1, 1, 1, 1), b), gold["window"])
    assert abs(got[0] - want) <= 1e-15
    assert R.mse(np.full((1, 1, 1, 1), a), np.full((1, 1, 1, 1), b))[0] == 0.25
    x = np.array([-1.0, -0.2, 0.3, 1.0], np.float32)
    assert np.array_equal(R.premap(x), ((x + np.float32(1)) / np.float32(2)).astype(np.float32))
    assert np.array_equal(R.premap(x, 0.0, 1.0), x)


def test_reconstruction_views_are_the_scripts_call(M):
    """layout "reference": calculate_ssim(x0, x_recon.permute(0, 2, 3, 1)) on x0 (B, 64, 64, 3) --
    Ch = 64 image rows, planes of (width 64, colour 3) -- read in place: checked on the wrapper's
    argument struct, nothing is launched (CPU tensors)."""
    import torch
    from encdiff_amd import ops
    B, H, W, Cc = 5, 64, 64, 3
    x0, xr = torch.zeros(B, H, W, Cc), torch.zeros(B, Cc, H, W)
    a, b = M.reconstruction_views(x0, xr, "reference")
    args = ops.recon_args(a, b, 1., 0.5)
    assert (args.n, args.ch, args.h, args.w) == (B, 64, 64, 3)
    assert list(args.sa) == [H * W * Cc, W * Cc, Cc, 1]          # x0 as it lies
    assert list(args.sb) == [Cc * H * W, W, 1, H * W]            # the NCHW reconstruction, permuted by strides
    assert (args.a, args.b) == (x0.data_ptr(), xr.data_ptr())    # no copies
    assert (args.pre_add, args.pre_mul) == (1.0, 0.5)
    assert a.shape == b.shape and torch.equal(b, xr.permute(0, 2, 3, 1))
    a, b = M.reconstruction_views(x0, xr, "nchw")
    args = ops.recon_args(a, b)
    assert (args.n, args.ch, args.h, args.w) == (B, 3, 64, 64)
    assert list(args.sa) == [H * W * Cc, 1, W * Cc, Cc] and list(args.sb) == [Cc * H * W, H * W, W, 1]
    assert (args.a, args.b) == (x0.data_ptr(), xr.data_ptr()) and (args.pre_add, args.pre_mul) == (0.0, 1.0)
    # a batch taken from a pool: x0 is itself a permuted view of gathered NCHW images
    img = torch.zeros(B, Cc, H, W)
    a, b = M.reconstruction_views(img.permute(0, 2, 3, 1), xr, "reference")
    assert list(ops.recon_args(a, b).sa) == [Cc * H * W, W, 1, H * W]


def test_python_refusals(M):
    """Every refusal comes before a launch: there is no device here, and a launch attempt would raise
    RuntimeError (no CPU fallback), not ValueError."""
    import torch
    x0, xr = torch.zeros(2, 8, 8, 3), torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="layout"):
        M.reconstruction_scores(x0, xr, layout="nhwc")
    with pytest.raises(ValueError, match=r"x0 \(B, H, W, C\)"):
        M.reconstruction_scores(x0, x0)
    with pytest.raises(ValueError, match=r"x0 \(B, H, W, C\)"):
        M.reconstruction_scores(x0[0], xr)
    with pytest.raises(ValueError, match="one shape"):
        M.ssim(xr, xr[:1])
    with pytest.raises(ValueError, match="one shape"):
        M.mse(xr[0], xr[0])
    with pytest.raises(ValueError, match="float32"):
        M.ssim(xr, xr.double())
    with pytest.raises(ValueError, match="every axis >= 1"):
        M.ssim(xr[:0], xr[:0])
    with pytest.raises(ValueError, match="torch tensors"):
        M.ssim(xr.numpy(), xr.numpy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.ssim(xr, xr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.reconstruction_scores(x0, xr)


def test_reconstruction_metrics_refusals():
    import torch
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self):  # the refusals come before the model is touched
            pass

    m = Bare()
    pool = torch.zeros(4, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="either pool or images"):
        m.reconstruction_metrics()
    with pytest.raises(ValueError, match="either pool or images"):
        m.reconstruction_metrics(pool=pool, images=pool.float())
    with pytest.raises(ValueError, match="layout"):
        m.reconstruction_metrics(pool=pool, layout="hwc")
    with pytest.raises(ValueError, match="uint8"):
        m.reconstruction_metrics(pool=pool.float())
    with pytest.raises(ValueError, match=r"\(N, H, W, C\)"):
        m.reconstruction_metrics(images=torch.zeros(4, 8, 8))
    with pytest.raises(ValueError, match="no images"):
        m.reconstruction_metrics(pool=pool, max_images=0)
    with pytest.raises(ValueError, match="batch_size"):
        m.reconstruction_metrics(pool=pool, batch_size=0)


def _args(L, **over):
    """A well-formed call: every pointer a made-up non-NULL address (the refusals dereference none)."""
    kw = dict(a=1 << 32, b=2 << 32, window=3 << 32, partial=4 << 32, ssim=5 << 32, mse=6 << 32,
              n=2, ch=3, h=16, w=16, pre_add=0.0, pre_mul=1.0)
    kw.update(over)
    return L.ReconArgs(**kw)


def test_abi_refusals():
    """NULL pointer: ENCDIFF_ERR_ARG; n, ch, h or w < 1, or n ch h w >= 2^31: ENCDIFF_ERR_SHAPE; each
    returned before anything is launched (there is no device here; the shape checks of a call with
    valid pointers come after the pointer checks, so every code below is what a launch-free return
    gives)."""
    import encdiff_amd._lib as L
    lib = L.lib
    assert lib.encdiff_ssim_mse(None, None) == ERR_ARG
    for miss in ("a", "b", "window", "partial", "ssim", "mse"):
        assert lib.encdiff_ssim_mse(C.byref(_args(L, **{miss: None})), None) == ERR_ARG, miss
    bad = [dict(n=0), dict(ch=0), dict(h=0), dict(w=0), dict(n=-1), dict(w=-5),
           dict(n=1 << 15, ch=1, h=1 << 8, w=1 << 8),          # exactly 2^31 elements
           dict(n=32768, ch=64, h=64, w=16), dict(n=2147483647, ch=2, h=1, w=1)]
    for b in bad:
        assert lib.encdiff_ssim_mse(C.byref(_args(L, **b)), None) == ERR_SHAPE, b
        nb = C.c_longlong(-7)
        assert lib.encdiff_ssim_mse_workspace(C.byref(_args(L, **b)), C.byref(nb)) == ERR_SHAPE, b
        assert nb.value == -7
    assert lib.encdiff_ssim_mse_workspace(None, C.byref(C.c_longlong())) == ERR_ARG
    assert lib.encdiff_ssim_mse_workspace(C.byref(_args(L)), None) == ERR_ARG


def test_workspace_sizes():
    """16 bytes per tile of a plane; the tile shape is the one of 16 x 16, 64 x 4 and 4 x 64 that
    covers the plane with the fewest tiles (16 x 16 on a tie).  Only n, ch, h, w are read."""
    from encdiff_amd import ops

    def tiles(h, w):
        return min(-(-h // th) * -(-w // tw) for th, tw in ((16, 16), (64, 4), (4, 64)))

    for n, ch, h, w in list(SHAPES.values()) + [(128, 64, 64, 3), (128, 3, 64, 64), (1, 1, 65, 4), (1, 1, 4, 65),
                                                  (1, 2, 3, 200), (1, 1, 1, 1), (2147483647, 1, 1, 1)]:
        assert ops.ssim_mse_workspace_bytes(n, ch, h, w) == 16 * n * ch * tiles(h, w), (n, ch, h, w)
    assert ops.ssim_mse_workspace_bytes(128, 64, 64, 3) == 16 * 128 * 64     # one 64 x 4 tile per 64 x 3 plane
    assert ops.ssim_mse_workspace_bytes(128, 3, 64, 64) == 16 * 128 * 3 * 16


def test_recon_args_layout_matches_c():
    """ReconArgs has exactly the C layout of EncdiffReconArgs (the gcc probe of test_abi.py, for this
    one struct)."""
    import encdiff_amd._lib as L
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){",
             'printf("size %zu\\n", sizeof(EncdiffReconArgs));']
    for fname, _ in L.ReconArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(EncdiffReconArgs, {fname}));')
    lines.append('printf("WINDOW_SIZE %d\\n", ENCDIFF_SSIM_WINDOW);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = []
    for line in out.strip().splitlines():
        field, val = line.split()
        if field == "size":
            assert C.sizeof(L.ReconArgs) == int(val)
        elif field == "WINDOW_SIZE":
            assert int(val) == 11
        else:
            assert getattr(L.ReconArgs, field).offset == int(val), field
            seen.append(field)
    assert seen == [f for f, _ in L.ReconArgs._fields_]
    assert L.ReconArgs.sa.size == 32 and L.ReconArgs.sb.size == 32
