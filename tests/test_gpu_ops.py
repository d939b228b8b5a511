"""Per-kernel numerics on the MI355X: every HIP op against a plain PyTorch fp32
reference of the same op, evaluated on the same (bf16-rounded) inputs.

Tolerances: bf16-output kernels rel-L2 <= 1e-2 (one bf16 rounding of the output,
fp32 accumulation); fp32-output kernels (weight gradients) rel-L2 <= 2e-3.
Attention is also tested per element, on every launch path, in test_gpu_attention.py.
The GEMM / implicit-im2col engine (every tile, split-K form, halo / WG3 / WGL kernel, paired and
grouped launch) is also tested per element, bitwise on exact integer cases, in test_gpu_gemm.py.
The fused SpatialTransformer kernels (every row tile, wave count, statistics and key-gradient form)
are also tested per element, stage by stage on their own saved tensors, in test_gpu_st.py.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = "cuda"


def rel(a, b):
    a = a.double(); b = b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    return ops


def bf(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).to(torch.bfloat16)


def nhwc(x, g):  # [pix][c] -> NCHW fp32
    return x.float().reshape(g.batch, g.h, g.w, -1).permute(0, 3, 1, 2)


def to_rows(x):  # NCHW -> [pix][c]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


@pytest.mark.parametrize("M,N,K", [(512, 256, 256), (1000, 72, 64), (32768, 64, 64), (130, 2048, 256),
                                   (128, 10240, 256), (2560, 128, 16)])
def test_linear(O, M, N, K):
    torch.manual_seed(0)
    x, w = bf(M, K), bf(N, K, scale=K ** -0.5)
    b = torch.randn(N, device=dev)
    r = bf(M, N)
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    O.linear_fwd(x, w, out, bias=b, resid=r)
    ref = x.float() @ w.float().t() + b + r.float()
    assert rel(out, ref) < 1e-2
    # fp32 output
    out32 = torch.empty(M, N, device=dev)
    O.linear_fwd(x, w, out32, bias=b, out_f32=True)
    assert rel(out32, x.float() @ w.float().t() + b) < 1e-4
    dy = bf(M, N)
    dx = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
    O.linear_dgrad(dy, w, dx)
    assert rel(dx, dy.float() @ w.float()) < 1e-2
    dw = torch.zeros(N, K, device=dev)
    db = torch.zeros(N, device=dev)
    O.linear_wgrad(dy, x, dw, db)
    assert rel(dw, dy.float().t() @ x.float()) < 2e-3
    assert rel(db, dy.float().sum(0)) < 2e-3
    # forced split-K: slab weight AND bias gradients accumulate (+=) reproducibly
    import encdiff_amd._lib as L
    for split in (1, 4):
        if split * N * (K + 1) > O.WS_FLOATS:
            continue
        dw2, db2 = dw.clone(), db.clone()
        outs = []
        for _ in range(2):
            a2, b2 = dw2.clone(), db2.clone()
            O.gemm(N, K, M, dy, dy.stride(0), x, x.stride(0), a2, K, a_mode=L.OPA_ROWM, b_mode=L.OPB_ROWN,
                   c_mode=L.OUT_F32_ACCUM, bias_grad=b2, split_k=split, tile=4)
            outs.append((a2, b2))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert rel(outs[0][0] - dw2, dy.float().t() @ x.float()) < 2e-3
        assert rel(outs[0][1] - db2, dy.float().sum(0)) < 2e-3


@pytest.mark.parametrize("split", [2, 8])
def test_split_k_workspace(O, split):
    """bf16-output GEMM with split-K: fp32 workspace partials + finalize (bias, resid)."""
    torch.manual_seed(11)
    M, N, K = 512, 256, 4608
    x, w = bf(M, K), bf(N, K, scale=K ** -0.5)
    b = torch.randn(N, device=dev)
    r = bf(M, N)
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    for _ in range(2):  # second call checks the workspace was left zeroed
        O.gemm(M, N, K, x, K, w, K, out, N, bias=b, resid=r, ld_resid=N, split_k=split, tile=4)
        assert rel(out, x.float() @ w.float().t() + b + r.float()) < 1e-2


@pytest.mark.parametrize("split", [2, 3, 8, 16])
@pytest.mark.parametrize("tile", [1, 4, 5])
def test_split_k_in_kernel_combine(O, tile, split):
    """Split-K slabs combined in the kernel by the last-arriving split (split_counters) vs the
    finalize pass: bitwise equal where the finalize also sums in split order (split <= 8), within
    fp32 rounding beyond; bf16 output with bias + residual and an fp32 accumulate output; the
    tickets are left zero; the input gradient of a 3x3 conv (paired with its weight gradient)."""
    import encdiff_amd._lib as L
    torch.manual_seed(12)
    M, N, K = 320, 192, 2304
    x, w = bf(M, K), bf(N, K, scale=K ** -0.5)
    b = torch.randn(N, device=dev)
    r = bf(M, N)
    outs = {}
    for fold in (False, True):
        O.SPLIT_FOLD = 2 if fold else 0
        try:
            o16 = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            O.gemm(M, N, K, x, K, w, K, o16, N, bias=b, resid=r, ld_resid=N, split_k=split, tile=tile)
            o32 = torch.full((M, N), 0.5, device=dev)
            O.gemm(M, N, K, x, K, w, K, o32, N, c_mode=L.OUT_F32_ACCUM, split_k=split, tile=tile)
            torch.cuda.synchronize()
        finally:
            O.SPLIT_FOLD = 1
        outs[fold] = (o16, o32)
    ref = x.float() @ w.float().t()
    assert rel(outs[True][0], ref + b + r.float()) < 1e-2
    assert rel(outs[True][1], ref + 0.5) < 1e-5
    if split <= 8:
        assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    assert rel(outs[True][1], outs[False][1]) < 1e-6
    assert int(O._counters().abs().sum()) == 0
    # paired conv backward whose input gradient is split: folded dgrad, deferred weight gradient
    from encdiff_amd.ops import Geom
    g = Geom(8, 4, 4)
    cin, cout = 256, 256
    xs, dy = bf(g.pixels, cin), bf(g.pixels, cout)
    wf = bf(cout, 9 * cin, scale=(9 * cin) ** -0.5)
    res = []
    for fold in (False, True):
        O.SPLIT_FOLD = 2 if fold else 0
        try:
            dw = torch.zeros(cout, 9 * cin, device=dev)
            dx = torch.empty(g.pixels, cin, device=dev, dtype=torch.bfloat16)
            O.gemm_pair(lambda off: O.conv3x3_wgrad_cl_args(dy, xs, g, cin, dw, None, 0, off),
                        lambda off: O.gemm_args(g.pixels, cin, 9 * cout, dy, cout, wf, 9 * cin, dx, cin,
                                                a_mode=L.OPA_IM2COL, b_mode=L.OPB_CONV_DGRAD,
                                                conv=L.ConvGeom(batch=8, h=4, w=4, cin=cout, resample=0, ld_src=cout),
                                                conv_cout=cout, split_k=split, tile=4, ws_offset=off))
            O.flush()
            torch.cuda.synchronize()
        finally:
            O.SPLIT_FOLD = 1
        res.append((dw, dx))
    assert torch.equal(res[0][0], res[1][0])
    if split <= 8:
        assert torch.equal(res[0][1], res[1][1])
    assert rel(res[1][1], res[0][1]) < 1e-2
    assert int(O._counters().abs().sum()) == 0


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_gemm_tiles(O, tile):
    """Every tile shape / LDS ring depth (tiles 5, 6: 4- and 3-deep rings; 7, 8: 128-deep k
    stages; 9, 10: 6- and 8-deep rings) on a ragged problem with a k-tile count that is not a
    multiple of the ring depth, split-K 1 and 3, on a 3x3 conv forward + input gradient, and (deep
    rings) a linear layer's paired weight / input gradient."""
    torch.manual_seed(3)
    M, N, K = 328, 200, 1000
    x, w = bf(M, K), bf(N, K, scale=K ** -0.5)
    ref = x.float() @ w.float().t()
    for split in (1, 3):
        out = torch.empty(M, N, device=dev)
        O.gemm(M, N, K, x, K, w, K, out, N, c_mode=O.L.OUT_F32, split_k=split, tile=tile)
        O.flush()
        assert rel(out, ref) < 1e-4, (tile, split)
    # implicit-im2col forward and input gradient (k-inner A, k-outer flipped-weight B)
    from encdiff_amd.ops import Geom
    g = Geom(3, 8, 8)
    cin, cout = 72, 200
    xs = bf(g.pixels, cin)
    wt = torch.randn(cout, cin, 3, 3, device=dev) / math.sqrt(9 * cin)
    wf = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).to(torch.bfloat16).contiguous()
    wq = wf.float().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    O.FORCE_TILE = tile
    try:
        y = torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16)
        O.conv3x3_fwd(xs, g, cin, wf, y)
        dy = bf(g.pixels, cout)
        dx = torch.empty(g.pixels, cin, device=dev, dtype=torch.bfloat16)
        O.conv3x3_dgrad(dy, g, wf, dx)
    finally:
        O.FORCE_TILE = 0
    xin = nhwc(xs, g).requires_grad_(True)
    ref = F.conv2d(xin, wq, padding=1)
    assert rel(nhwc(y, g), ref) < 1e-2, tile
    ref.backward(nhwc(dy, g))
    assert rel(nhwc(dx, g), xin.grad) < 1e-2, tile
    if tile in (5, 9, 10):  # paired linear backward, both halves on the deep ring
        L = O.L
        Mt, Ct, Ci = 2048, 64, 96
        dyl, xl, wl = bf(Mt, Ct), bf(Mt, Ci), bf(Ct, Ci)
        for split in (1, 4, 16):
            dw = torch.full((Ct, Ci), 0.25, device=dev)
            dxl = torch.empty(Mt, Ci, device=dev, dtype=torch.bfloat16)
            O.gemm_pair(lambda off: O.gemm_args(Ct, Ci, Mt, dyl, Ct, xl, Ci, dw, Ci, a_mode=L.OPA_ROWM,
                                                b_mode=L.OPB_ROWN, c_mode=L.OUT_F32_ACCUM, split_k=split, tile=tile,
                                                ws_offset=off),
                        lambda off: O.gemm_args(Mt, Ci, Ct, dyl, Ct, wl, Ci, dxl, Ci, b_mode=L.OPB_ROWN, split_k=1,
                                                tile=tile, ws_offset=off))
            O.flush()
            torch.cuda.synchronize()
            assert rel(dw, dyl.float().t() @ xl.float() + 0.25) < 1e-5, (tile, split)
            assert rel(dxl, dyl.float() @ wl.float()) < 1e-2, (tile, split)


HALO_TWIN = {16: 4, 17: 2, 18: 1, 22: 3}  # halo tile -> the ring tile of the same BM x BN


@pytest.mark.parametrize("tile", [16, 17, 18, 19, 20, 21, 22, 23])
@pytest.mark.parametrize("B,H,cin,cout,mode", [(4, 16, 64, 64, 0), (4, 8, 128, 96, 0), (2, 16, 192, 64, 0),
                                               (2, 16, 128, 64, 2), (2, 32, 32, 32, 3), (2, 64, 8, 32, 0),
                                               (3, 16, 32, 128, 4), (2, 32, 24, 32, 0)])
def test_conv_halo_tiles(O, tile, B, H, cin, cout, mode):
    """Halo tiles (16-23): the workgroup's whole conv-input window staged once in LDS.  Forward
    (3x3 pad 1, nearest-up, VQ stride-2, Encoder4 k4 s2) and the 3x3 input gradient vs torch fp32,
    and bitwise equal to the LDS-ring tile of the same shape (same k order, same MFMA sequence).
    Shapes the window does not fit (LDS) or whose tile straddles image rows are refused."""
    import encdiff_amd._lib as L
    from encdiff_amd.ops import Geom
    torch.manual_seed(9)
    g = Geom(B, H, H)
    k4 = mode == 4
    src_h = 2 * H if mode in (3, 4) else (H // 2 if mode == 2 else H)
    gs = Geom(B, src_h, src_h)
    T = 16 if k4 else 9
    x = bf(gs.pixels, cin)
    wf = bf(cout, T * cin, scale=(T * cin) ** -0.5)
    kh = 4 if k4 else 3
    wq = wf.float().reshape(cout, kh, kh, cin).permute(0, 3, 1, 2)
    bias = torch.randn(cout, device=dev)
    cg = L.ConvGeom(batch=B, h=H, w=H, cin=cin, resample=mode, ld_src=cin)

    def run(t, c_mode=L.OUT_BF16):
        out = torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16 if c_mode == L.OUT_BF16 else torch.float32)
        O.gemm(g.pixels, cout, T * cin, x, cin, wf, T * cin, out, cout, a_mode=L.OPA_IM2COL, c_mode=c_mode,
               conv=cg, bias=bias, split_k=1, tile=t)
        return out
    if not O.halo_fits(tile, B, H, H, cin, mode):  # the host mirror and the library agree on refusals
        with pytest.raises(L.HipError):
            run(tile)
        return
    y = run(tile)
    xin = nhwc(x, gs)
    if mode == 2:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    if mode == 3:
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wq, bias, stride=2)
    elif mode == 4:
        ref = F.conv2d(xin, wq, bias, stride=2, padding=1)
    else:
        ref = F.conv2d(xin, wq, bias, padding=1)
    assert rel(nhwc(y, g), ref) < 1e-2
    y32 = run(tile, L.OUT_F32)
    assert rel(nhwc(y32, g), ref) < 1e-4
    if tile in HALO_TWIN:
        assert torch.equal(y32, run(HALO_TWIN[tile], L.OUT_F32))
    if mode != 0:
        return
    # input gradient: dY im2col through the window, flipped weights
    dy = bf(g.pixels, cout)
    cgd = L.ConvGeom(batch=B, h=H, w=H, cin=cout, resample=0, ld_src=cout)

    def drun(t):
        dx = torch.empty(g.pixels, cin, device=dev)
        O.gemm(g.pixels, cin, 9 * cout, dy, cout, wf, 9 * cin, dx, cin, a_mode=L.OPA_IM2COL,
               b_mode=L.OPB_CONV_DGRAD, c_mode=L.OUT_F32, conv=cgd, conv_cout=cout, split_k=1, tile=t)
        return dx
    if not O.halo_fits(tile, B, H, H, cout, 0):
        with pytest.raises(L.HipError):
            drun(tile)
        return
    dx = drun(tile)
    xr = nhwc(x, gs).requires_grad_(True)
    F.conv2d(xr, wq, None, padding=1).backward(nhwc(dy, g))
    assert rel(nhwc(dx, g), xr.grad) < 1e-4
    if tile in HALO_TWIN:
        assert torch.equal(dx, drun(HALO_TWIN[tile]))


@pytest.mark.parametrize("tile", [16, 17, 22])
@pytest.mark.parametrize("split", [2, 4])
@pytest.mark.parametrize("B,H,cin,cout,mode", [(32, 4, 256, 256, 0), (32, 4, 512, 256, 0), (64, 2, 512, 256, 0),
                                               (16, 8, 256, 128, 0), (32, 4, 256, 256, 2), (16, 2, 768, 256, 0)])
def test_conv_halo_split_k(O, tile, split, B, H, cin, cout, mode):
    """Halo tiles with split-K over source-channel slices (the small-image convs: a 64-row tile is
    whole 4x4 / 2x2 images, each split stages its channel slice of their windows once and runs all
    9 taps over it): forward (bf16 out through the slab finalize, and the in-kernel combine) and the
    input gradient vs torch fp32; bitwise equal to the same split on the LDS-ring tile is not
    expected (different k order), so the bound is the fp32 one."""
    import encdiff_amd._lib as L
    from encdiff_amd.ops import Geom
    torch.manual_seed(19)
    g = Geom(B, H, H)
    gs = Geom(B, H // 2, H // 2) if mode == 2 else g
    x = bf(gs.pixels, cin)
    wf = bf(cout, 9 * cin, scale=(9 * cin) ** -0.5)
    wq = wf.float().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    bias = torch.randn(cout, device=dev)
    cg = L.ConvGeom(batch=B, h=H, w=H, cin=cin, resample=mode, ld_src=cin)
    if not O.halo_fits(tile, B, H, H, cin, mode, split):
        # the host mirror declines: the library must decline too (an error, no launch) -- the
        # planner relies on the two agreeing
        out = torch.empty(g.pixels, cout, device=dev)
        with pytest.raises(L.HipError):
            O.gemm(g.pixels, cout, 9 * cin, x, cin, wf, 9 * cin, out, cout, a_mode=L.OPA_IM2COL, c_mode=L.OUT_F32,
                   conv=cg, split_k=split, tile=tile)
        return
    xin = nhwc(x, gs)
    if mode == 2:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    ref = F.conv2d(xin, wq, bias, padding=1)
    for c_mode, fold, tol in ((L.OUT_F32, False, 1e-4), (L.OUT_BF16, False, 1e-2), (L.OUT_BF16, True, 1e-2)):
        out = torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16 if c_mode == L.OUT_BF16 else torch.float32)
        O.gemm(g.pixels, cout, 9 * cin, x, cin, wf, 9 * cin, out, cout, a_mode=L.OPA_IM2COL, c_mode=c_mode,
               conv=cg, bias=bias, split_k=split, tile=tile, fold=fold)
        assert rel(nhwc(out, g), ref) < tol, (c_mode, fold)
    if mode != 0 or not O.halo_fits(tile, B, H, H, cout, 0, split):
        return
    dy = bf(g.pixels, cout)
    cgd = L.ConvGeom(batch=B, h=H, w=H, cin=cout, resample=0, ld_src=cout)
    dx = torch.empty(g.pixels, cin, device=dev)
    O.gemm(g.pixels, cin, 9 * cout, dy, cout, wf, 9 * cin, dx, cin, a_mode=L.OPA_IM2COL, b_mode=L.OPB_CONV_DGRAD,
           c_mode=L.OUT_F32, conv=cgd, conv_cout=cout, split_k=split, tile=tile)
    xr = nhwc(x, gs).requires_grad_(True)
    F.conv2d(xr, wq, None, padding=1).backward(nhwc(dy, g))
    assert rel(nhwc(dx, g), xr.grad) < 1e-4


def test_linear_strided_views(O):
    """q/k/v slices of a fused [M][3C] projection output are strided views."""
    torch.manual_seed(1)
    M, C = 4096, 128
    x = bf(M, 3 * C)[:, C:2 * C]
    w = bf(C, C, scale=C ** -0.5)
    outbuf = torch.zeros(M, 2 * C, device=dev, dtype=torch.bfloat16)
    out = outbuf[:, C:]
    O.linear_fwd(x, w, out)
    assert rel(out, x.float() @ w.float().t()) < 1e-2
    assert outbuf[:, :C].abs().max().item() == 0


def test_conv3x3_down2_is_rejected(O):
    """AvgPool2d-then-conv is pooled by the executor (one resample launch), not in the GEMM gather."""
    import encdiff_amd._lib as L
    from encdiff_amd.ops import Geom
    g = Geom(2, 8, 8)
    x = bf(2 * 16 * 16, 64)
    wf = bf(64, 9 * 64)
    out = torch.empty(g.pixels, 64, device=dev, dtype=torch.bfloat16)
    with pytest.raises(L.HipError):
        O.conv3x3_fwd(x, g, 64, wf, out, resample=L.RESAMPLE_DOWN2)


@pytest.mark.parametrize("B,H,cin,cout,mode", [(4, 16, 64, 64, 0), (2, 16, 192, 64, 0), (3, 8, 128, 256, 0),
                                               (2, 8, 32, 32, 3), (2, 8, 256, 256, 2), (8, 2, 256, 256, 0),
                                               (2, 4, 512, 256, 0), (2, 32, 64, 32, 3)])
def test_conv3x3(O, B, H, cin, cout, mode):
    from encdiff_amd.ops import Geom
    torch.manual_seed(2)
    g = Geom(B, H, H)
    src_h = 2 * H if mode in (1, 3) else (H // 2 if mode == 2 else H)
    gs = Geom(B, src_h, src_h)
    x = bf(gs.pixels, cin)
    wt = torch.randn(cout, cin, 3, 3, device=dev) / math.sqrt(9 * cin)
    wf = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).to(torch.bfloat16).contiguous()
    wq = wf.float().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    bias = torch.randn(cout, device=dev)
    out = torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16)
    O.conv3x3_fwd(x, g, cin, wf, out, bias=bias, resample=mode)
    xin = nhwc(x, gs)
    if mode == 1:
        xin = F.avg_pool2d(xin, 2)
    elif mode == 2:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    xin = xin.to(torch.bfloat16).float() if mode == 1 else xin
    xin.requires_grad_(True)
    wq.requires_grad_(True)
    if mode == 3:  # VQ Downsample: F.pad(0,1,0,1) + conv k3 s2 p0 (forward only: the VQ encoder is frozen)
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wq, bias, stride=2)
        assert rel(nhwc(out, g), ref) < 1e-2
        return
    ref = F.conv2d(xin, wq, bias, padding=1)
    assert rel(nhwc(out, g), ref) < 1e-2
    dy = bf(g.pixels, cout)
    ref.backward(nhwc(dy, g))
    # dgrad at the conv resolution
    dx = torch.empty(g.pixels, cin, device=dev, dtype=torch.bfloat16)
    O.conv3x3_dgrad(dy, g, wf, dx)
    assert rel(nhwc(dx, g), xin.grad) < 1e-2
    dw = torch.zeros(cout, cin, 3, 3, device=dev)
    db = torch.zeros(cout, device=dev)
    O.conv3x3_wgrad(dy, x, g, cin, dw, db, resample=mode)
    assert rel(dw, wq.grad) < 5e-3
    assert rel(db, nhwc(dy, g).sum((0, 2, 3))) < 2e-3
    # channels-last weight gradient ([co][kh][kw][ci], the arena layout)
    dwc = torch.zeros(cout, 9 * cin, device=dev)
    db2 = torch.zeros(cout, device=dev)
    O.conv3x3_wgrad_cl(dy, x, g, cin, dwc, db2, resample=mode)
    assert rel(dwc.view(cout, 3, 3, cin).permute(0, 3, 1, 2), wq.grad) < 5e-3
    assert rel(db2, db) < 1e-5


@pytest.mark.parametrize("B,H,cin,cout,mode", [(128, 16, 64, 64, 0), (16, 16, 192, 64, 0), (32, 16, 128, 128, 2),
                                                (128, 8, 128, 128, 0), (64, 8, 384, 128, 0), (128, 4, 256, 256, 0),
                                                (16, 4, 512, 256, 2), (8, 8, 64, 32, 0)])
@pytest.mark.parametrize("tile", [32, 33, 34])
def test_conv3x3_wgrad_wg3(O, B, H, cin, cout, mode, tile, monkeypatch):
    """The 3x3 weight-gradient kernel (gemm_wg3.h WG3, tile 32) vs a torch fp32 reference and vs the
    split-K GEMM form: dW (channels-last, accumulated onto a nonzero dW) and the bias gradient;
    then two paired backward launches in a row (the first's finalize deferred into the second).
    The heuristic WG3 plan is what is tested here (no tuned-table override, ops.TABLE_WG)."""
    monkeypatch.setattr(O, "TABLE_WG", 0)
    from encdiff_amd.ops import Geom
    from encdiff_amd import _lib as L
    torch.manual_seed(11)
    g = Geom(B, H, H)
    gs = Geom(B, H // 2, H // 2) if mode == 2 else g
    x, dy = bf(gs.pixels, cin), bf(g.pixels, cout)
    sp = O.wg3_split(B, H, H, cout, cin, mode, cout, cin, L.OUT_F32_ACCUM, tile=tile)
    assert sp is not None, "shape expected to be WG3-eligible"
    xin = nhwc(x, gs)
    if mode == 2:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    w0 = torch.zeros(cout, cin, 3, 3, device=dev, requires_grad=True)
    F.conv2d(xin, w0, padding=1).backward(nhwc(dy, g))
    ref = w0.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    init = torch.randn(cout, 9 * cin, device=dev)
    got = {}
    for wg3 in (1, 0):
        O.WG3, O.WG3_TILE = wg3, tile
        try:
            a = O.conv3x3_wgrad_cl_args(dy, x, g, cin, init.clone(), None, mode)
            assert (a.tile in (32, 33, 34)) == bool(wg3) and (not wg3 or a.split_k == sp)
            dw, db = init.clone(), torch.full((cout,), 0.5, device=dev)
            O.conv3x3_wgrad_cl(dy, x, g, cin, dw, db, resample=mode)
            torch.cuda.synchronize()
        finally:
            O.WG3, O.WG3_TILE = 1, 32
        got[wg3] = (dw, db)
    dw, db = got[1]
    assert rel(dw - init, ref) < 2e-3, rel(dw - init, ref)
    assert rel(db - 0.5, nhwc(dy, g).sum((0, 2, 3))) < 2e-3
    assert rel(dw, got[0][0]) < 1e-5 and rel(db, got[0][1]) < 1e-5
    # two paired backward launches: WG3 weight gradients, the first finalize rides in the second
    wf = bf(cout, 9 * cin, scale=(9 * cin) ** -0.5)
    dws = [init.clone(), init.clone()]
    dxs = [torch.empty(g.pixels, cin, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    O.WG3_TILE = tile
    try:
        for i in range(2):
            O.conv3x3_bwd_cl(dy, g, wf, x, cin, dws[i], dxs[i], resample=mode)
        O.flush()
    finally:
        O.WG3_TILE = 32
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(dws[i], got[1][0]) or rel(dws[i], got[1][0]) < 1e-6


@pytest.mark.parametrize("T,cout,cin", [(32768, 64, 64), (8192, 128, 128), (2048, 256, 256), (32768, 512, 64),
                                         (8192, 1024, 128), (2048, 2048, 256), (256, 64, 128), (2048, 192, 64)])
def test_linear_wgrad_wgl(O, T, cout, cin, monkeypatch):
    """The linear weight-gradient kernel (gemm_wgl.h WGL, tile 36) vs a torch fp32 reference and vs
    the split-K GEMM form (dW accumulated onto a nonzero dW, bias gradient), then two paired
    backward launches in a row (input gradient in the same grid, the first finalize deferred)."""
    monkeypatch.setattr(O, "TABLE_WG", 0)  # the heuristic WGL plan (no tuned-table override)
    torch.manual_seed(12)
    dy, x = bf(T, cout), bf(T, cin)
    sp = O.wgl_split(cout, cin, T, cout, cin, O.L.OUT_F32_ACCUM)
    assert sp is not None
    ref = dy.float().t() @ x.float()
    init = torch.randn(cout, cin, device=dev)
    got = {}
    for wgl in (1, 0):
        O.WGL = 2 * wgl
        try:
            a = O.linear_wgrad_args(dy, x, init.clone())
            assert (a.tile == 36) == bool(wgl) and (not wgl or a.split_k == sp)
            dw, db = init.clone(), torch.full((cout,), 0.5, device=dev)
            O.linear_wgrad(dy, x, dw, db)
            O.flush()
            torch.cuda.synchronize()
        finally:
            O.WGL = 1
        got[wgl] = (dw, db)
    dw, db = got[1]
    assert rel(dw - init, ref) < 2e-3, rel(dw - init, ref)
    assert rel(db - 0.5, dy.float().sum(0)) < 2e-3
    assert rel(dw, got[0][0]) < 1e-5 and rel(db, got[0][1]) < 1e-5
    w = bf(cout, cin, scale=cout ** -0.5)
    dws = [init.clone(), init.clone()]
    dxs = [torch.empty(T, cin, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    O.WGL = 2  # (the step's default pairs only square layers on WGL)
    try:
        for i in range(2):
            O.linear_bwd(dy, w, x, dxs[i], dws[i])
        O.flush()
        torch.cuda.synchronize()
    finally:
        O.WGL = 1
    for i in range(2):
        assert torch.equal(dws[i], got[1][0]) or rel(dws[i], got[1][0]) < 1e-6
        assert rel(dxs[i], dy.float() @ w.float()) < 1e-2


def test_table_wg_tile33_pair(O, monkeypatch):
    """with ENCDIFF_TABLE_WG on (the default), a tuned table entry naming the 8-wave WG3
    kernel (tile 33) with its split overrides the heuristic; the paired backward then launches the
    riding finalize of the previous layer as a launch of its own.  Two paired layers in a row vs
    torch fp32; and a table entry that is invalid for the problem (a split that does not divide the
    batch into whole stages) falls back to a valid plan instead of raising."""
    from encdiff_amd.ops import Geom
    torch.manual_seed(23)
    B, H, cin, cout = 32, 16, 64, 64
    g = Geom(B, H, H)
    x, dy = bf(g.pixels, cin), bf(g.pixels, cout)
    key = O.plan_key(cout, 9 * cin, g.pixels, O.L.OPA_ROWM, O.L.OPB_IM2COL, O.L.OUT_F32_ACCUM, 0, H)
    table = dict(O._tile_table())
    table[key] = [33, 4, 0.0]
    monkeypatch.setattr(O, "_TILES", table)
    monkeypatch.setattr(O, "TABLE_WG", 1)
    a = O.conv3x3_wgrad_cl_args(dy, x, g, cin, torch.zeros(cout, 9 * cin, device=dev))
    assert (a.tile, a.split_k) == (33, 4)
    w0 = torch.zeros(cout, cin, 3, 3, device=dev, requires_grad=True)
    F.conv2d(nhwc(x, g), w0, padding=1).backward(nhwc(dy, g))
    ref = w0.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    wf = bf(cout, 9 * cin, scale=(9 * cin) ** -0.5)
    dws = [torch.zeros(cout, 9 * cin, device=dev) for _ in range(2)]
    dxs = [torch.empty(g.pixels, cin, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    for i in range(2):
        O.conv3x3_bwd_cl(dy, g, wf, x, cin, dws[i], dxs[i])
    O.flush()
    torch.cuda.synchronize()
    for i in range(2):
        assert rel(dws[i], ref) < 2e-3, rel(dws[i], ref)
    # an entry whose split does not divide this batch into whole 8-wave stage sets: not taken
    table[key] = [33, 64, 0.0]
    a = O.conv3x3_wgrad_cl_args(dy, x, g, cin, torch.zeros(cout, 9 * cin, device=dev))
    assert (a.tile, a.split_k) != (33, 64)
    dw = torch.zeros(cout, 9 * cin, device=dev)
    O.conv3x3_wgrad_cl(dy, x, g, cin, dw)
    O.flush()
    torch.cuda.synchronize()
    assert rel(dw, ref) < 2e-3


def test_wgrad_group(O):
    """Grouped weight gradients (encdiff_wgrad_group_*): one grid over every body the group has --
    WG3 at 16 / 8 / 4 (resample none and nearest-up), WGL, the generic 64x64 tile for 2x2 convs and
    for narrow / short-K linears -- each problem whole (no split-K), vs torch fp32 references;
    dW and the bias gradient accumulate onto nonzero values; a second launch of the same planned
    group is bitwise the first (one ordered sum per output element)."""
    from encdiff_amd.ops import Geom
    torch.manual_seed(21)
    convs = [(64, 16, 64, 64, 0), (16, 16, 128, 64, 2), (32, 8, 128, 128, 0), (16, 8, 256, 128, 2),
             (32, 4, 256, 256, 0), (16, 4, 512, 256, 2), (32, 2, 256, 256, 0), (8, 2, 512, 256, 2)]
    lins = [(8192, 64, 64), (2048, 512, 128), (4096, 256, 1024), (128, 1024, 256), (2560, 64, 16), (384, 200, 72)]
    grp = O.WgradGroup()
    cases, keep = [], []  # keep: operands stay alive until the deferred group launch
    O.group_begin(grp)
    try:
        for B, H, cin, cout, mode in convs:
            g = Geom(B, H, H)
            gs = Geom(B, H // 2, H // 2) if mode == 2 else g
            x, dy = bf(gs.pixels, cin), bf(g.pixels, cout)
            xin = nhwc(x, gs)
            if mode == 2:
                xin = F.interpolate(xin, scale_factor=2, mode="nearest")
            w0 = torch.zeros(cout, cin, 3, 3, device=dev, requires_grad=True)
            F.conv2d(xin, w0, padding=1).backward(nhwc(dy, g))
            ref = w0.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)
            dw, db = torch.randn(cout, 9 * cin, device=dev), torch.randn(cout, device=dev)
            cases.append((dw, dw.clone(), ref, db, db.clone(), nhwc(dy, g).sum((0, 2, 3))))
            keep += [x, dy]
            O.conv3x3_wgrad_cl(dy, x, g, cin, dw, db, resample=mode)
        for T, cout, cin in lins:
            dy, x = bf(T, cout), bf(T, cin)
            dw, db = torch.randn(cout, cin, device=dev), torch.randn(cout, device=dev)
            cases.append((dw, dw.clone(), dy.float().t() @ x.float(), db, db.clone(), dy.float().sum(0)))
            keep += [x, dy]
            O.linear_wgrad(dy, x, dw, db)
        assert len(grp.probs) == len(cases)
        O.group_end()
    finally:
        O.group_begin(None)
    torch.cuda.synchronize()
    for i, (dw, w0, ref, db, b0, rb) in enumerate(cases):
        assert rel(dw - w0, ref) < 2e-3, (i, rel(dw - w0, ref))
        assert rel(db - b0, rb) < 2e-3, (i, rel(db - b0, rb))
    first = [(c[0].clone(), c[3].clone()) for c in cases]
    # relaunch the same planned group (the executors replay it every step): identical sums
    for dw, w0, _, db, b0, _ in cases:
        dw.copy_(w0)
        db.copy_(b0)
    arr = list(grp._plans.values())
    assert len(arr) == 1
    host, devb = arr[0][:2]
    O.check(O.lib.encdiff_wgrad_group_launch(O.C.addressof(host), devb.data_ptr(), O._s()), "group")
    torch.cuda.synchronize()
    for i, ((dw, _, _, db, _, _), (f_dw, f_db)) in enumerate(zip(cases, first)):
        if not (torch.equal(dw, f_dw) and torch.equal(db, f_db)):
            bad = (dw != f_dw).nonzero()
            print(f"case {i} {tuple(dw.shape)}: {bad.shape[0]} dW elements differ, first {bad[:4].tolist()} last "
                  f"{bad[-4:].tolist()}, max |d| {(dw - f_dw).abs().max().item():.3e}, vs ref first "
                  f"{rel(f_dw - cases[i][1], cases[i][2]):.3e} second {rel(dw - cases[i][1], cases[i][2]):.3e}; "
                  f"db differ {(db != f_db).sum().item()}")
    for (dw, _, _, db, _, _), (f_dw, f_db) in zip(cases, first):
        assert torch.equal(dw, f_dw) and torch.equal(db, f_db)


@pytest.mark.parametrize("C,H,film,silu,eps", [(64, 16, True, True, 1e-5), (192, 16, False, True, 1e-5),
                                                (384, 8, True, True, 1e-5), (256, 4, False, False, 1e-6),
                                                (512, 2, True, True, 1e-5), (64, 64, True, True, 1e-5),
                                                (128, 8, False, True, 1e-5)])
def test_groupnorm(O, C, H, film, silu, eps):
    from encdiff_amd.ops import Geom
    torch.manual_seed(3)
    B = 6
    g = Geom(B, H, H)
    x = (torch.randn(g.pixels, C, device=dev) * 2 + 0.5).to(torch.bfloat16)
    gamma = 1 + 0.1 * torch.randn(C, device=dev)
    beta = 0.1 * torch.randn(C, device=dev)
    E = torch.randn(B, 2 * C + 32, device=dev) * 0.3 if film else None
    y = torch.empty_like(x)
    stats = torch.empty(B, 32, 2, device=dev)
    O.groupnorm_fwd(x, g, gamma, beta, y, stats, eps, silu, film=E, ld_film=E.shape[1] if film else 0)
    xr = nhwc(x, g).requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    Er = E.clone().requires_grad_(True) if film else None
    ref = F.group_norm(xr, 32, gr, br, eps)
    if film:
        ref = ref * (1 + Er[:, :C, None, None]) + Er[:, C:2 * C, None, None]
    if silu:
        ref = F.silu(ref)
    assert rel(nhwc(y, g), ref) < 1e-2
    dy = bf(g.pixels, C)
    ref.backward(nhwc(dy, g))
    dx = torch.empty_like(x)
    dgp = torch.empty(B, C, device=dev)
    dbp = torch.empty(B, C, device=dev)
    dE = torch.zeros(B, 2 * C + 32, device=dev) if film else None
    O.groupnorm_bwd(x, g, gamma, beta, stats, eps, silu, dy, dx, dgp, dbp, film=E,
                    ld_film=E.shape[1] if film else 0, dfilm=dE, ld_dfilm=dE.shape[1] if film else 0)
    assert rel(nhwc(dx, g), xr.grad) < 1e-2
    assert rel(dgp.sum(0), gr.grad) < 2e-3
    assert rel(dbp.sum(0), br.grad) < 2e-3
    if film:
        assert rel(dE[:, :2 * C], Er.grad[:, :2 * C]) < 2e-3
    if silu:
        # training form: the forward also stores silu'(z) (bf16); y is bitwise the plain forward's,
        # and the backward reading it matches the reference like the recomputing one
        ds = torch.empty_like(x)
        y2 = torch.empty_like(x)
        O.groupnorm_fwd(x, g, gamma, beta, y2, stats, eps, silu, film=E, ld_film=E.shape[1] if film else 0, dsilu=ds)
        assert torch.equal(y2, y)
        z = F.group_norm(nhwc(x, g).float(), 32, gamma, beta, eps)
        if film:
            z = z * (1 + E[:, :C, None, None]) + E[:, C:2 * C, None, None]
        sz = torch.sigmoid(z)
        assert rel(nhwc(ds, g), sz * (1 + z * (1 - sz))) < 1e-2
        dx2 = torch.empty_like(x)
        dgp2, dbp2 = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
        dE2 = torch.zeros(B, 2 * C + 32, device=dev) if film else None
        O.groupnorm_bwd(x, g, gamma, beta, stats, eps, silu, dy, dx2, dgp2, dbp2, film=E,
                        ld_film=E.shape[1] if film else 0, dfilm=dE2, ld_dfilm=dE2.shape[1] if film else 0, dsilu=ds)
        assert rel(nhwc(dx2, g), xr.grad) < 1e-2
        assert rel(dgp2.sum(0), gr.grad) < 5e-3
        assert rel(dbp2.sum(0), br.grad) < 5e-3
        if film:
            assert rel(dE2[:, :2 * C], Er.grad[:, :2 * C]) < 5e-3


@pytest.mark.parametrize("rows,C", [(32768, 64), (8192, 128), (2048, 256), (512, 256), (1000, 128),
                                    (1000, 512)])
def test_layernorm(O, rows, C):
    torch.manual_seed(4)
    x = (torch.randn(rows, C, device=dev) + 0.3).to(torch.bfloat16)
    gamma = 1 + 0.1 * torch.randn(C, device=dev)
    beta = 0.1 * torch.randn(C, device=dev)
    y = torch.empty_like(x)
    st = torch.empty(rows, 2, device=dev)
    O.layernorm_fwd(x, gamma, beta, y, st)
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), gr, br, 1e-5)
    assert rel(y, ref) < 1e-2
    dy = bf(rows, C)
    ref.backward(dy.float())
    dx = bf(rows, C)
    base = dx.float().clone()
    parts = O.layernorm_parts(rows, C)
    dgp = torch.empty(parts, C, device=dev)
    dbp = torch.empty(parts, C, device=dev)
    O.layernorm_bwd(x, gamma, st, dy, dx, dgp, dbp, accumulate=True)
    assert rel(dx.float() - base, xr.grad) < 2e-2
    assert rel(dgp.sum(0), gr.grad) < 2e-3
    assert rel(dbp.sum(0), br.grad) < 2e-3


@pytest.mark.parametrize("B,heads,sq,sk,dh,cross", [(4, 8, 256, 256, 8, False), (4, 8, 64, 64, 16, False),
                                                    (4, 8, 16, 16, 32, False), (4, 8, 4, 4, 32, False),
                                                    (4, 8, 256, 20, 8, True), (4, 8, 16, 20, 32, True),
                                                    # configs[4] wide UNet: S=1024 at dh 16, dh 64 levels
                                                    (2, 8, 1024, 1024, 16, False), (4, 8, 64, 64, 64, False),
                                                    (4, 8, 16, 40, 64, True)])
def test_attention(O, B, heads, sq, sk, dh, cross):
    _attention_case(O, B, heads, sq, sk, dh, cross, fp8=False)


@pytest.mark.parametrize("qscale", [1.0, 12.0], ids=["bound", "running_max"])
@pytest.mark.parametrize("B,heads,sq,sk,dh", [(4, 8, 256, 256, 8), (4, 8, 64, 64, 16), (4, 8, 16, 20, 32),
                                              (4, 8, 256, 20, 8), (2, 4, 48, 40, 16)])
def test_attention_fwd_score_bound(O, B, heads, sq, sk, dh, qscale):
    """Forward softmax offsets: rows whose Cauchy-Schwarz score bound |q| max|k| scale log2e is small
    use it as a fixed offset (no running max); large scores (q x 12) take the online-max path.  Both:
    output and natural-log LSE vs torch fp32 (the LSE feeds the backward)."""
    torch.manual_seed(9)
    C = heads * dh
    q = (torch.randn(B * sq, C, device=dev) * qscale).to(torch.bfloat16)
    kv = bf(B * sk, 2 * C)
    k, v = kv[:, :C], kv[:, C:]
    o = torch.empty(B * sq, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B * heads, sq, device=dev)
    O.attention_fwd(q, k, v, o, lse, B, heads, sq, sk, dh)

    def split(t, s):
        return t.float().reshape(B, s, heads, dh).permute(0, 2, 1, 3).reshape(B * heads, s, dh)
    sc = split(q, sq) @ split(k, sk).transpose(1, 2) * dh ** -0.5
    ref = (sc.softmax(-1) @ split(v, sk)).reshape(B, heads, sq, dh).permute(0, 2, 1, 3).reshape(B * sq, C)
    lref = torch.logsumexp(sc, -1)
    bound = (split(q, sq).norm(dim=-1, keepdim=True) * split(k, sk).norm(dim=-1).amax(-1)[:, None, None]
             * dh ** -0.5 / math.log(2)).amax().item()
    print(f"max row score bound (log2) {bound:.1f}: out rel-L2 {rel(o, ref):.3e}, "
          f"lse max-abs {(lse - lref).abs().max().item():.3e}")
    assert rel(o, ref) < 1e-2
    assert (lse - lref).abs().max().item() < 2e-3 * max(1.0, lref.abs().max().item())


@pytest.mark.parametrize("B,heads,sq,sk,dh,cross", [(2, 8, 1024, 1024, 16, False), (4, 8, 256, 256, 32, False),
                                                    (4, 8, 64, 64, 64, False), (4, 8, 256, 20, 16, True)])
def test_attention_fp8_scores(O, B, heads, sq, sk, dh, cross):
    """fp8 (OCP e4m3) QK^T (configs[4]'s S = 1024 level): vs a torch fp32 reference whose scores
    use q, k rounded to float8_e4m3fn and whose gradient products use the bf16 q, k (what the
    kernel computes), plus the distance to plain bf16 attention."""
    _attention_case(O, B, heads, sq, sk, dh, cross, fp8=True)


def _attention_case(O, B, heads, sq, sk, dh, cross, fp8):
    torch.manual_seed(5)
    C = heads * dh
    if cross:
        q = bf(B * sq, C)
        kv = bf(B * sk, 2 * C)
        k, v = kv[:, :C], kv[:, C:]
    else:
        qkv = bf(B * sq, 3 * C)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    o = torch.empty(B * sq, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B * heads, sq, device=dev)
    O.attention_fwd(q, k, v, o, lse, B, heads, sq, sk, dh, fp8=fp8)

    def split(t, s):
        return t.float().reshape(B, s, heads, dh).permute(0, 2, 1, 3).reshape(B * heads, s, dh)

    def merge(t, s):
        return t.reshape(B, heads, s, dh).permute(0, 2, 1, 3).reshape(B * s, C)
    d_o = bf(B * sq, C)
    dq = torch.empty_like(o)
    dkv = torch.empty(B * sk, 2 * C, device=dev, dtype=torch.bfloat16)
    O.attention_bwd(q, k, v, o, lse, d_o, dq, dkv[:, :C], dkv[:, C:], B, heads, sq, sk, dh, fp8=fp8)
    if fp8:
        qs, ks, vs, gs = split(q, sq), split(k, sk), split(v, sk), split(d_o, sq)
        e4 = torch.float8_e4m3fn
        att = (qs.to(e4).float() @ ks.to(e4).float().transpose(1, 2) * dh ** -0.5).softmax(-1)
        ref = att @ vs
        dp = gs @ vs.transpose(1, 2)
        dsc = att * (dp - (dp * att).sum(-1, keepdim=True))
        want = dict(dq=dsc @ ks * dh ** -0.5, dk=dsc.transpose(1, 2) @ qs * dh ** -0.5, dv=att.transpose(1, 2) @ gs)
        plain = (qs @ ks.transpose(1, 2) * dh ** -0.5).softmax(-1) @ vs
        print(f"fp8 scores: out rel-L2 vs e4m3 reference {rel(o, merge(ref, sq)):.3e}, vs bf16 attention "
              f"{rel(o, merge(plain, sq)):.3e}")
        assert rel(o, merge(ref, sq)) < 1e-2
        assert rel(split(dq, sq), want["dq"]) < 2e-2
        assert rel(split(dkv[:, :C], sk), want["dk"]) < 2e-2
        assert rel(split(dkv[:, C:], sk), want["dv"]) < 2e-2
        return
    qr, kr, vr = (split(q, sq).requires_grad_(True), split(k, sk).requires_grad_(True),
                  split(v, sk).requires_grad_(True))
    att = (qr @ kr.transpose(1, 2) * dh ** -0.5).softmax(-1)
    ref = att @ vr
    refm = merge(ref, sq)
    assert rel(o, refm) < 1e-2
    refm.backward(d_o.float())
    assert rel(split(dq, sq), qr.grad) < 2e-2
    assert rel(split(dkv[:, :C], sk), kr.grad) < 2e-2
    assert rel(split(dkv[:, C:], sk), vr.grad) < 2e-2


def test_elementwise(O):
    from encdiff_amd.ops import Geom
    import encdiff_amd._lib as L
    torch.manual_seed(6)
    M, n = 4096, 256
    f = bf(M, 2 * n)
    y = torch.empty(M, n, device=dev, dtype=torch.bfloat16)
    O.geglu_fwd(f, y)
    fr = f.float().requires_grad_(True)
    a, gt = fr.chunk(2, -1)
    ref = a * F.gelu(gt)
    assert rel(y, ref) < 1e-2
    dy = bf(M, n)
    ref.backward(dy.float())
    df = torch.empty_like(f)
    O.geglu_bwd(f, dy, df)
    assert rel(df, fr.grad) < 1e-2
    # resample down / up and adjoints
    g = Geom(3, 8, 8)
    x = bf(3 * 16 * 16, 64)
    yd = torch.empty(g.pixels, 64, device=dev, dtype=torch.bfloat16)
    O.resample(x, yd, g, L.RESAMPLE_DOWN2)
    assert rel(nhwc(yd, g), F.avg_pool2d(nhwc(x, Geom(3, 16, 16)), 2)) < 1e-2
    gu = Geom(3, 16, 16)
    xu = bf(3 * 64, 64)
    yu = torch.empty(gu.pixels, 64, device=dev, dtype=torch.bfloat16)
    O.resample(xu, yu, gu, L.RESAMPLE_UP2)
    assert rel(nhwc(yu, gu), F.interpolate(nhwc(xu, Geom(3, 8, 8)), scale_factor=2, mode="nearest")) < 1e-2
    # adjoint of down: grad at 16x16 from dy at 8x8
    xs = nhwc(x, Geom(3, 16, 16)).requires_grad_(True)
    dyd = bf(g.pixels, 64)
    F.avg_pool2d(xs, 2).backward(nhwc(dyd, g))
    dxs = torch.empty_like(x)
    O.resample_bwd(dyd, dxs, Geom(3, 16, 16), L.RESAMPLE_DOWN2)
    assert rel(nhwc(dxs, Geom(3, 16, 16)), xs.grad) < 1e-2
    xs2 = nhwc(xu, Geom(3, 8, 8)).requires_grad_(True)
    dyu = bf(gu.pixels, 64)
    F.interpolate(xs2, scale_factor=2, mode="nearest").backward(nhwc(dyu, gu))
    dxu = torch.empty_like(xu)
    O.resample_bwd(dyu, dxu, Geom(3, 8, 8), L.RESAMPLE_UP2)
    assert rel(nhwc(dxu, Geom(3, 8, 8)), xs2.grad) < 1e-2


def test_small_convs(O):
    from encdiff_amd.ops import Geom
    torch.manual_seed(7)
    B = 5
    g = Geom(B, 16, 16)
    x = torch.randn(B, 3, 16, 16, device=dev)
    w = torch.randn(64, 3, 3, 3, device=dev) * 0.2
    b = torch.randn(64, device=dev)
    y = torch.empty(g.pixels, 64, device=dev, dtype=torch.bfloat16)
    O.small_conv_in_fwd(x, g, w, b, y)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    ref = F.conv2d(x, wr, br, padding=1)
    assert rel(nhwc(y, g), ref) < 1e-2
    dy = bf(g.pixels, 64)
    ref.backward(nhwc(dy, g))
    dw = torch.zeros_like(w); db = torch.zeros_like(b)
    O.small_conv_in_wgrad(x, g, w, dy, dw, db)
    assert rel(dw, wr.grad) < 2e-3 and rel(db, br.grad) < 2e-3
    # output conv 64 -> 3
    h = bf(g.pixels, 64)
    w2 = torch.randn(3, 64, 3, 3, device=dev) * 0.05
    b2 = torch.randn(3, device=dev)
    out = torch.empty(B, 3, 16, 16, device=dev)
    O.small_conv_out_fwd(h, g, w2, b2, out)
    hr = nhwc(h, g).requires_grad_(True)
    w2r = w2.clone().requires_grad_(True); b2r = b2.clone().requires_grad_(True)
    ref2 = F.conv2d(hr, w2r, b2r, padding=1)
    assert rel(out, ref2) < 1e-4
    d2 = torch.randn(B, 3, 16, 16, device=dev)
    ref2.backward(d2)
    dh = torch.empty_like(h)
    dw2 = torch.zeros_like(w2); db2 = torch.zeros_like(b2)
    O.small_conv_out_bwd(h, g, w2, d2, dh, dw2, db2)
    assert rel(nhwc(dh, g), hr.grad) < 1e-2
    assert rel(dw2, w2r.grad) < 2e-3 and rel(db2, b2r.grad) < 2e-3


@pytest.mark.parametrize("cin,H", [(64, 16), (128, 16), (128, 32), (96, 8), (512, 4)])
def test_small_conv_out_channels(O, cin, H):
    """Output conv cin -> 3 forward (lane-group kernel for power-of-two cin/8, the per-pixel
    kernel otherwise) and input gradient, against torch fp32."""
    from encdiff_amd.ops import Geom
    torch.manual_seed(cin + H)
    B = 3
    g = Geom(B, H, H)
    h = bf(g.pixels, cin)
    w2 = torch.randn(3, cin, 3, 3, device=dev) * 0.05
    b2 = torch.randn(3, device=dev)
    out = torch.empty(B, 3, H, H, device=dev)
    O.small_conv_out_fwd(h, g, w2, b2, out)
    hr = nhwc(h, g).requires_grad_(True)
    ref = F.conv2d(hr, w2, b2, padding=1)
    assert rel(out, ref) < 1e-4
    d2 = torch.randn(B, 3, H, H, device=dev)
    ref.backward(d2)
    dh = torch.empty_like(h)
    O.small_conv_out_bwd(h, g, w2, d2, dh, None, None)
    assert rel(nhwc(dh, g), hr.grad) < 1e-2


def test_diffusion_math(O):
    from oracle import encdiff_oracle as OR
    torch.manual_seed(8)
    B = 16
    t = torch.randint(0, 1000, (B,), device=dev)
    emb = torch.empty(B, 64, device=dev, dtype=torch.bfloat16)
    O.timestep_embedding(t, 64, emb)
    assert rel(emb, OR.timestep_embedding(t.cpu(), 64).to(dev)) < 1e-2
    sch = {k: v.to(dev) for k, v in OR.sched_fp32(OR.register_schedule()).items()}
    x0 = torch.randn(B, 3, 16, 16, device=dev)
    eps = torch.randn_like(x0)
    xt = torch.empty_like(x0)
    O.q_sample(x0, eps, t, sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"], xt)
    assert rel(xt, OR.q_sample(sch, x0, t, eps)) < 1e-6
    pred = torch.randn_like(x0).requires_grad_(True)
    out2 = torch.empty(2, device=dev)
    grad = torch.empty_like(x0)
    O.l1_loss(pred.detach(), eps, t, sch["lvlb_weights"], out2, grad)
    loss, ld = OR.p_losses_from_output(sch, pred, eps, t, logvar=torch.zeros(1000, device=dev))
    loss.backward()
    assert abs(out2[0].item() - loss.item()) < 1e-5 and abs(out2[1].item() - ld["loss_vlb"].item()) < 1e-5 * max(
        1, abs(ld["loss_vlb"].item()))
    assert rel(grad, pred.grad) < 1e-6
    z = torch.randn_like(x0)
    xp = torch.empty_like(x0); px = torch.empty_like(x0)
    O.ddim_step(xt, pred.detach(), z, 0.5, 0.7, 0.1, math.sqrt(0.5), xp, px)
    rx, rp = OR.ddim_step(xt.cpu(), pred.detach().cpu(), 0.5, 0.7, 0.1, math.sqrt(0.5), z.cpu())
    assert rel(xp.cpu(), rx) < 1e-6 and rel(px.cpu(), rp) < 1e-6


def test_adamw_ema_pack_reduce(O):
    from oracle import encdiff_oracle as OR
    import encdiff_amd._lib as L
    torch.manual_seed(9)
    n = 4096
    p = torch.randn(n, device=dev); g = torch.randn(n, device=dev)
    m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev)
    ema = p.clone()
    rp, rm, rv = p.cpu().clone(), m.cpu().clone(), v.cpu().clone()
    rema = {"x": ema.cpu().clone()}
    nu = 0
    for step in range(1, 4):
        hy = torch.tensor(O.adamw_hyper(1e-3, step, ema_one_minus_decay=1 - min(0.9999, (1 + step) / (10 + step))),
                          device=dev)
        O.adamw_ema(p, g, m, v, hy, ema=ema, ema_n=n - 100)
        rp, rm, rv = OR.adamw_step(rp, g.cpu(), rm, rv, step, 1e-3)
        new, nu = OR.ema_update(rema, {"x": rp}, nu)
        rema["x"][: n - 100] = new["x"][: n - 100]
    assert (p.cpu() - rp).abs().max().item() < 1e-6
    assert (ema.cpu() - rema["x"]).abs().max().item() < 1e-6
    # pack conv weight [co][ci][3][3] -> [co][tap][ci] bf16
    w = torch.randn(32, 16, 3, 3, device=dev)
    dst = torch.zeros(32 * 9 * 16 + 100, device=dev, dtype=torch.bfloat16)
    jobs = (L.PackJob * 2)(L.PackJob(src_off=0, dst_off=0, rows=32, cols=144, kind=1, cin=16),
                           L.PackJob(src_off=0, dst_off=32 * 144, rows=1, cols=100, kind=0, cin=0))
    jt = torch.frombuffer(bytearray(jobs), dtype=torch.uint8).to(dev)
    O.pack_weights(w.reshape(-1), dst, jt, 2)
    assert torch.equal(dst[: 32 * 144].reshape(32, 3, 3, 16), w.permute(0, 2, 3, 1).to(torch.bfloat16))
    assert torch.equal(dst[32 * 144:], w.reshape(-1)[:100].to(torch.bfloat16))
    part = torch.randn(7, 50, device=dev)
    idx = torch.randperm(200, device=dev)[:50].to(torch.int32)
    gr = torch.zeros(200, device=dev)
    O.reduce_partials(part, 50, 7, 50, idx, gr)
    ref = torch.zeros(200, device=dev)
    ref[idx.long()] = part.sum(0)
    assert rel(gr, ref) < 1e-6


def test_gather_images_u8(O):
    """GPU-resident dataset gather + ToTensor/Normalize/CHW == oracle bit-exact, with the
    device step counter walking the epoch (and wrapping) on its own."""
    from encdiff_amd.data import ImagePool
    from oracle import encdiff_oracle as Orc
    pool = ImagePool.synthetic(37, 8, dev, seed=3)
    out = torch.empty(8, 3, 64, 64, device=dev)
    for s in range(pool.steps_per_epoch + 2):
        pool.draw(out)
        k = s % pool.steps_per_epoch
        idx = pool.perm[k * 8:(k + 1) * 8].cpu()
        ref = Orc.images_to_input(pool.images.cpu(), idx)
        assert torch.equal(out.cpu(), ref)
    assert int(pool.step) == pool.steps_per_epoch + 2


def test_step_prologue(O):
    """encdiff_step_prologue (one launch in front of a training step): zero jobs clear exactly their
    regions (strided 2-D views included), t ~ U{0..T-1} and noise ~ N(0, 1) (ddpm_enc.py:1041,
    :1184) with the right moments, the Philox stream is a function of (seed, counter) only
    (same counter -> same draw; counter and data step advance by one per launch, also under graph
    replay), and the ticket is left at zero."""
    from encdiff_amd import ops as P
    pro = P.StepPrologue(dev, seed=1234)
    big = torch.randn(3, 1000, device=dev)
    side = torch.randn(16, 192, device=dev)
    keep = side.clone()
    pro.set_jobs([big, side[:, 64:128]])
    t = torch.empty(4096, dtype=torch.long, device=dev)
    noise = torch.empty(128, 3, 16, 16, device=dev)
    step = torch.zeros(1, dtype=torch.long, device=dev)
    pro(t, noise, timesteps=1000, data_step=step)
    torch.cuda.synchronize()
    assert int(big.abs().sum()) == 0
    assert side[:, 64:128].abs().sum().item() == 0
    assert torch.equal(side[:, :64], keep[:, :64]) and torch.equal(side[:, 128:], keep[:, 128:])
    assert int(t.min()) >= 0 and int(t.max()) <= 999 and len(torch.unique(t)) > 900
    assert abs(t.float().mean().item() - 499.5) < 15
    n = noise.flatten().double()
    assert abs(n.mean().item()) < 0.02 and abs(n.std().item() - 1) < 0.02
    assert abs(((n.abs() < 1).double().mean()).item() - 0.6827) < 0.01
    assert int(pro.counter) == 1 and int(step) == 1 and int(pro.done) == 0
    t1, n1 = t.clone(), noise.clone()
    pro(t, noise, timesteps=1000, data_step=step)
    assert not torch.equal(t, t1) and not torch.equal(noise, n1)
    pro.counter.fill_(0)
    pro(t, noise, timesteps=1000)
    assert torch.equal(t, t1) and torch.equal(noise, n1)
    # graph replay advances the counter by itself
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            pro(t, noise, timesteps=1000, data_step=step)
    torch.cuda.current_stream().wait_stream(s)
    c0, s0 = int(pro.counter), int(step)
    g.replay()
    a = noise.clone()
    g.replay()
    torch.cuda.synchronize()
    assert int(pro.counter) == c0 + 2 and int(step) == s0 + 2 and not torch.equal(a, noise)


@pytest.mark.parametrize("B,units", [(128, 20), (600, 40), (1100, 20)])
def test_encoder_head(O, B, units):
    """Encoder4's flatten + Linear head (openaimodel_enc.py:1012-1013) on HIP vs torch fp32: u, the
    trunk gradient dr (bf16) and dW / db -- including batches past the old LDS-staging limit
    (B >= 410 at 40 units), where du is staged in chunks."""
    from encdiff_amd import _lib as L, ops as P
    g = torch.Generator().manual_seed(B + units)
    d = 128
    r = torch.randn(B * 16, d, generator=g).to(dev)                       # NHWC rows of the 4x4 trunk output
    W = (torch.randn(units, d * 16, generator=g) * 0.02).to(dev)
    bias = torch.randn(units, generator=g).to(dev)
    flat = r.view(B, 16, d).permute(0, 2, 1).reshape(B, d * 16)           # NCHW flatten (k = c * 16 + p)
    u = torch.empty(B, units, device=dev)
    L.check(L.lib.encdiff_encoder_head_fwd(r.data_ptr(), r.stride(0), B, d, W.data_ptr(), bias.data_ptr(), units,
                                           u.data_ptr(), u.stride(0), P._s()), "head_fwd")
    assert rel(u, flat @ W.t() + bias) < 1e-5
    du = torch.randn(B, units, generator=g).to(dev)
    dr = torch.empty(B * 16, d, device=dev, dtype=torch.bfloat16)
    dW = torch.zeros_like(W)
    db = torch.zeros_like(bias)
    L.check(L.lib.encdiff_encoder_head_bwd(r.data_ptr(), r.stride(0), B, d, W.data_ptr(), units, du.data_ptr(),
                                           du.stride(0), dr.data_ptr(), dr.stride(0), dW.data_ptr(), db.data_ptr(),
                                           P._s()), "head_bwd")
    dflat = du @ W
    want_dr = dflat.view(B, d, 16).permute(0, 2, 1).reshape(B * 16, d)
    r_dr, r_dw, r_db = rel(dr.float(), want_dr), rel(dW, du.t() @ flat), rel(db, du.sum(0))
    print(f"head B={B} units={units}: dr {r_dr:.2e} dW {r_dw:.2e} db {r_db:.2e}")
    assert r_dr < 1e-2 and r_dw < 1e-5 and r_db < 1e-5


@pytest.mark.parametrize("B", [128, 50])
def test_encoder_warp(O, B):
    """Encoder4.warp on HIP (fp32) vs the as-is torch modules (fp32) on the same params:
    outputs, d u and every per-unit weight/bias gradient."""
    import copy
    from encdiff_amd.arena import ParamArena
    from encdiff_amd.ldm.modules.diffusionmodules.openaimodel_enc import Encoder4
    torch.manual_seed(9)
    enc = Encoder4(128, 16, 20).to(dev)
    ref = copy.deepcopy(enc)
    arena = ParamArena([("cond_stage_model." + n, p) for n, p in enc.named_parameters()], dev)
    enc.bind_arena(arena, "cond_stage_model.")
    u = torch.randn(B, 20, device=dev, requires_grad=True)
    u2 = u.detach().clone().requires_grad_(True)
    out, outr = enc.warp(u), ref.warp(u2)
    assert rel(out, outr) < 1e-5
    g = torch.randn_like(out)
    arena.grad.zero_()
    out.backward(g)
    outr.backward(g)
    assert rel(u.grad, u2.grad) < 1e-5
    for (n, p), (_, pr) in zip(enc.net.named_parameters(), ref.net.named_parameters()):
        assert rel(p.grad, pr.grad) < 1e-4, n


@pytest.mark.parametrize("force", [0, 7])
@pytest.mark.parametrize("kind,M,C,K", [("lin", 32768, 64, 64), ("lin", 2048, 256, 256), ("lin", 8192, 128, 512),
                                         ("conv", 16, 64, 64), ("conv", 8, 256, 256), ("conv", 4, 256, 512)])
def test_gemm_pair_matches_two_launches(O, kind, M, C, K, force):
    """encdiff_gemm_pair (weight + input gradient of one layer in ONE launch) is bitwise
    identical to the two separate GEMMs, whatever tiles / split-K the plan picks (force=7:
    both with 128-deep k stages, the paired kernel's KB1 = KB2 = 128 instantiation)."""
    O.FORCE_TILE = force
    try:
        _pair_case(O, kind, M, C, K)
    finally:
        O.FORCE_TILE = 0


def _pair_case(O, kind, M, C, K):
    import encdiff_amd._lib as L
    from encdiff_amd.ops import Geom
    torch.manual_seed(3)
    outs = []
    if kind == "lin":
        dy, x, w = bf(M, C), bf(M, K), bf(C, K, scale=K ** -0.5)
        for pair in (False, True):
            dw = torch.ones(C, K, device=dev)
            db = torch.ones(C, device=dev)
            dx = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
            if pair:
                O.linear_bwd(dy, w, x, dx, dw, db)
                O.flush()  # the weight-gradient finalize is deferred into the next pair / flush
            else:
                O.linear_wgrad(dy, x, dw, db)
                O.linear_dgrad(dy, w, dx)
            outs.append((dw, db, dx))
        assert rel(outs[1][0] - 1, dy.float().t() @ x.float()) < 2e-3
        assert rel(outs[1][2], dy.float() @ w.float()) < 1e-2
    else:
        g = Geom(128, M, M)
        cin, cout = K, C
        dy, x, wf = bf(g.pixels, cout), bf(g.pixels, cin), bf(cout, 9 * cin, scale=(9 * cin) ** -0.5)
        for pair in (False, True):
            dw = torch.zeros(cout, 9 * cin, device=dev)
            db = torch.zeros(cout, device=dev)
            dx = torch.empty(g.pixels, cin, device=dev, dtype=torch.bfloat16)
            if pair:
                O.conv3x3_bwd_cl(dy, g, wf, x, cin, dw, dx, db)
                O.flush()
            else:
                O.conv3x3_wgrad_cl(dy, x, g, cin, dw, db)
                O.conv3x3_dgrad(dy, g, wf, dx)
            outs.append((dw, db, dx))
        ref_dx = F.conv_transpose2d(nhwc(dy, g), wf.float().view(cout, 3, 3, cin).permute(0, 3, 1, 2), padding=1)
        assert rel(nhwc(outs[1][2], g), ref_dx) < 1e-2
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H,C,relu", [(32, 128, True), (8, 128, False), (4, 128, True), (16, 64, True)])
def test_batchnorm_train_fwd_bwd(O, H, C, relu):
    """BatchNorm2d.train() (+ReLU) on NHWC bf16 rows vs torch fp32 on the same bf16 input; the
    ReLU mask is evaluated on identical inputs, so the backward is pinned tightly too."""
    import ctypes
    import encdiff_amd._lib as L
    torch.manual_seed(5)
    B = 16
    rows = B * H * H
    x = (torch.randn(rows, C, device=dev) * 2 + 0.5).to(torch.bfloat16)
    gamma = torch.rand(C, device=dev) + 0.5
    beta = torch.randn(C, device=dev) * 0.2
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    part = torch.empty(L.lib.encdiff_batchnorm_partials_floats(rows, C), device=dev)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = L.BatchNormArgs(rows=rows, c=C, eps=1e-5, momentum=0.1, relu=int(relu), x=x.data_ptr(), ldx=C,
                        gamma=gamma.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(), ldy=C, mean=mean.data_ptr(),
                        rstd=rstd.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
                        partials=part.data_ptr(), counter=cnt.data_ptr())
    L.check(L.lib.encdiff_batchnorm_fwd(ctypes.byref(a), s), "bn fwd")
    bn = torch.nn.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xr = nhwc(x, Geom_(B, H)).requires_grad_(True)
    ref = bn(xr)
    ref = torch.relu(ref) if relu else ref
    assert rel(nhwc(y, Geom_(B, H)), ref) < 1e-2
    assert rel(rm, bn.running_mean) < 1e-4 and rel(rv, bn.running_var) < 1e-4
    assert int(cnt.item()) == 0
    dy = bf(rows, C)
    ref.backward(nhwc(dy, Geom_(B, H)))
    dx = torch.empty_like(x)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    a.dy, a.lddy, a.dx, a.lddx, a.dgamma, a.dbeta = dy.data_ptr(), C, dx.data_ptr(), C, dg.data_ptr(), db.data_ptr()
    L.check(L.lib.encdiff_batchnorm_bwd(ctypes.byref(a), s), "bn bwd")
    assert rel(nhwc(dx, Geom_(B, H)), xr.grad) < 2e-2
    assert rel(dg, bn.weight.grad) < 2e-3 and rel(db, bn.bias.grad) < 2e-3


def Geom_(B, H):
    from encdiff_amd.ops import Geom
    return Geom(B, H, H)


@pytest.mark.parametrize("parity", [True, False])
@pytest.mark.parametrize("Hout,cin,cout", [(32, 8, 128), (16, 128, 128), (4, 128, 128)])
def test_conv4x4s2(O, Hout, cin, cout, parity):
    """Conv2d(k4, s2, p1) forward, input gradient (transposed im2col mode: by output parity,
    K4S2_TP, or all 16 taps, K4S2_T) and weight gradient vs torch fp32 on the same bf16
    operands; the parity mode also with split-K slabs (rows remapped by the finalize)."""
    torch.manual_seed(6)
    B = 8
    g = Geom_(B, Hout)
    gi = Geom_(B, 2 * Hout)
    x = bf(gi.pixels, cin)
    w = torch.randn(cout, cin, 4, 4, device=dev) * (16 * cin) ** -0.5
    wf = w.permute(0, 2, 3, 1).reshape(cout, 16 * cin).to(torch.bfloat16).contiguous()
    wr = wf.float().view(cout, 4, 4, cin).permute(0, 3, 1, 2)
    bias = torch.randn(cout, device=dev)
    out = torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16)
    O.conv4x4s2_fwd(x, g, cin, wf, out, bias=bias)
    ref = F.conv2d(nhwc(x, gi), wr, bias, stride=2, padding=1)
    assert rel(nhwc(out, g), ref) < 1e-2
    dy = bf(g.pixels, cout)
    dw = torch.zeros(cout, 16 * cin, device=dev)
    db = torch.zeros(cout, device=dev)
    dx = torch.empty(gi.pixels, cin, device=dev, dtype=torch.bfloat16)
    O.K4S2_PARITY = parity
    try:
        O.conv4x4s2_bwd_cl(dy, g, wf, x, cin, dw, dx, db)
    finally:
        O.K4S2_PARITY = True
    O.flush()
    xr = nhwc(x, gi).requires_grad_(True)
    wrr = wr.clone().requires_grad_(True)
    F.conv2d(xr, wrr, None, stride=2, padding=1).backward(nhwc(dy, g))
    assert rel(nhwc(dx, gi), xr.grad) < 1e-2
    if parity:
        import encdiff_amd._lib as L
        dx2 = torch.empty_like(dx)
        O.gemm(gi.pixels, cin, 4 * cout, dy, cout, wf, 16 * cin, dx2, cin, a_mode=L.OPA_IM2COL,
               b_mode=L.OPB_CONV_DGRAD, conv=L.ConvGeom(batch=B, h=gi.h, w=gi.w, cin=cout,
                                                        resample=L.RESAMPLE_K4S2_TP, ld_src=cout),
               conv_cout=cout, split_k=3, tile=4)
        assert rel(nhwc(dx2, gi), xr.grad) < 1e-2
    assert rel(dw.view(cout, 4, 4, cin).permute(0, 3, 1, 2), wrr.grad) < 2e-3
    assert rel(db, dy.float().sum(0)) < 2e-3


def test_gemm_pair_chain_deferred_finalize(O):
    """A chain of paired backward launches: each weight gradient's split-K finalize runs inside
    the NEXT pair's launch (ping-pong workspace halves), the last one at flush().  Bitwise equal
    to unpaired launches."""
    torch.manual_seed(4)
    shapes = [(32768, 64, 64), (8192, 128, 512), (2048, 256, 256), (32768, 192, 64), (512, 256, 1024)]
    ins = [(bf(M, C), bf(M, K), bf(C, K, scale=K ** -0.5)) for M, C, K in shapes]
    res = []
    for pair in (False, True):
        O.PAIR = pair
        try:
            outs = []
            for (dy, x, w), (M, C, K) in zip(ins, shapes):
                dw = torch.zeros(C, K, device=dev)
                db = torch.zeros(C, device=dev)
                dx = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
                O.linear_bwd(dy, w, x, dx, dw, db)
                outs += [dw, db, dx]
            O.flush()
        finally:
            O.PAIR = True
        res.append(outs)
    for a, b in zip(*res):
        assert torch.equal(a, b)
    for (dy, x, w), k in zip(ins, range(0, 15, 3)):
        assert rel(res[1][k], dy.float().t() @ x.float()) < 2e-3


@pytest.mark.parametrize("M,C,inner", [(4096, 64, 256), (1000, 128, 512), (256, 256, 1024)])
def test_geglu_fused(O, M, C, inner):
    """GEGLU in the GEMM epilogues (proj: f and y = f_v * gelu(f_g); next layer's input
    gradient: df) equals the separate ew kernels bitwise, and torch fp32 within bf16 tolerance."""
    torch.manual_seed(9)
    x = bf(M, C)
    w1 = bf(2 * inner, C, scale=C ** -0.5)
    b1 = torch.randn(2 * inner, device=dev) * 0.1
    w2 = bf(C, inner, scale=inner ** -0.5)
    dy = bf(M, C)
    outs = {}
    for fused in (True, False):
        O.GEGLU_FUSED = fused
        try:
            f = torch.empty(M, 2 * inner, device=dev, dtype=torch.bfloat16)
            y = torch.empty(M, inner, device=dev, dtype=torch.bfloat16)
            O.linear_fwd_geglu(x, w1, f, y, bias=b1)
            df = torch.empty_like(f)
            d_a = torch.empty_like(y)
            dw = torch.zeros(C, inner, device=dev)
            db = torch.zeros(C, device=dev)
            O.linear_bwd_geglu(dy, w2, y, f, df, dw, db, d_a=d_a)
            O.flush()
        finally:
            O.GEGLU_FUSED = True
        outs[fused] = (f, y, df, dw, db)
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    f, y, df, dw, db = outs[True]
    fr = x.float() @ w1.float().t() + b1
    assert rel(f, fr) < 1e-2
    fv, fg = f.float()[:, :inner], f.float()[:, inner:]
    assert rel(y, fv * F.gelu(fg)) < 1e-2
    fvr, fgr = fv.clone().requires_grad_(True), fg.clone().requires_grad_(True)
    (fvr * F.gelu(fgr)).backward((dy.float() @ w2.float()).to(torch.bfloat16).float())
    assert rel(df[:, :inner], fvr.grad) < 1e-2 and rel(df[:, inner:], fgr.grad) < 1e-2


@pytest.mark.parametrize("H,C,silu,film", [(16, 64, True, True), (16, 192, False, False), (8, 384, True, True),
                                         (64, 32, True, False), (32, 64, False, False)])
def test_groupnorm_from_producer_stats(O, H, C, silu, film):
    """A GEMM's epilogue segment sums (gn_stats) feed GroupNorm forward: same output and saved
    statistics as the reducing kernel up to fp32 summation order; also for a channel slice of
    a wider (concat) buffer."""
    from encdiff_amd.ops import Geom
    torch.manual_seed(12)
    B = 16
    g = Geom(B, H, H)
    K = 96
    xin = bf(g.pixels, K)
    w = bf(C, K, scale=K ** -0.5)
    bias = torch.randn(C, device=dev)
    wide = torch.zeros(g.pixels, C + 64, device=dev, dtype=torch.bfloat16)
    stw = torch.full((2 * g.pixels // 64, C + 64), float("nan"), device=dev)
    x = wide[:, 64:]
    O.linear_fwd(xin, w, x, bias=bias, gn_stats=stw[:, 64:])
    gam = torch.randn(C, device=dev)
    bet = torch.randn(C, device=dev)
    fl = torch.randn(B, 2 * C, device=dev) * 0.2 if film else None
    outs = []
    for st_in in (None, stw[:, 64:]):
        y = torch.empty(g.pixels, C, device=dev, dtype=torch.bfloat16)
        st = torch.empty(B * 32 * 2, device=dev)
        O.groupnorm_fwd(x, g, gam, bet, y, st, 1e-5, silu, film=fl, ld_film=2 * C if film else 0, in_stats=st_in)
        outs.append((y, st))
    assert rel(outs[1][1], outs[0][1]) < 1e-5
    assert rel(outs[1][0], outs[0][0]) < 1e-2
    assert (outs[1][0].float() - outs[0][0].float()).abs().max().item() < 0.05
    xf = nhwc(x, g)
    ref = F.group_norm(xf, 32, gam, bet, 1e-5)
    if film:
        ref = ref * (1 + fl[:, :C, None, None]) + fl[:, C:, None, None]
    if silu:
        ref = F.silu(ref)
    assert rel(nhwc(outs[1][0], g), ref) < 1e-2


@pytest.mark.parametrize("B,H,cin,cout,split,resid,film,alpha", [
    (128, 2, 256, 256, 8, "sep", False, 1.0), (8, 4, 256, 256, 16, None, True, 1.0),
    (16, 8, 128, 128, 2, "inplace", True, 1.0), (8, 16, 64, 64, 4, None, False, 1.0),
    (8, 2, 256, 256, 32, "inplace", False, 1.0), (8, 4, 256, 256, 16, "sep", True, 0.7),
    (8, 2, 256, 256, 32, None, False, 1.3)])
def test_groupnorm_from_deferred_finalize(O, B, H, cin, cout, split, resid, film, alpha):
    """encdiff_gemm_ex with the finalize deferred + GroupNorm forward combining the slabs
    (x_from) vs encdiff_gemm (tile kernel + finalize pass) + GroupNorm: the conv output x, the
    normalised output and the saved statistics bitwise equal (<= 8 slabs in one ordered sum,
    deeper splits in four z-groups, alpha != 1 with a bias -- the two combine copies are built
    without FMA contraction -- separate and in-place residual)."""
    import ctypes as C
    from encdiff_amd import _lib as L
    from encdiff_amd.ops import Geom, _conv_geom
    torch.manual_seed(31)
    g = Geom(B, H, H)
    a = bf(g.pixels, cin)
    w = bf(cout, 9 * cin, scale=(9 * cin) ** -0.5)
    bias = torch.randn(cout, device=dev) * 0.1
    r = bf(g.pixels, cout)
    gam = torch.randn(cout, device=dev)
    bet = torch.randn(cout, device=dev)
    fl = torch.randn(B, 2 * cout, device=dev) * 0.2 if film else None
    fold = O.SPLIT_FOLD
    O.SPLIT_FOLD = 0  # slabs for a finalize pass, not the in-kernel combine
    outs = []
    try:
        for defer in (False, True):
            x = r.clone() if resid == "inplace" else torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16)
            rs = x if resid == "inplace" else (r if resid == "sep" else None)
            args = O.gemm_args(g.pixels, cout, 9 * cin, a, cin, w, 9 * cin, x, cout, a_mode=L.OPA_IM2COL,
                               conv=_conv_geom(g, cin, L.RESAMPLE_NONE, a), bias=bias, resid=rs,
                               ld_resid=cout if rs is not None else 0, split_k=split, tile=4, alpha=alpha)
            assert args.split_k == split and not args.split_counters
            planned = C.c_int(-1)
            O.check(O.lib.encdiff_gemm_ex(C.byref(args), int(defer), C.byref(planned), O._s()), "gemm_ex")
            assert planned.value == int(defer)
            y = torch.empty(g.pixels, cout, device=dev, dtype=torch.bfloat16)
            st = torch.empty(B * 32 * 2, device=dev)
            O.groupnorm_fwd(x, g, gam, bet, y, st, 1e-5, True, film=fl, ld_film=2 * cout if film else 0,
                            x_from=args if defer else None)
            torch.cuda.synchronize()
            outs.append((x, y, st))
    finally:
        O.SPLIT_FOLD = fold
    for u, v in zip(outs[0], outs[1]):
        assert torch.equal(u, v)
    xr = alpha * F.conv2d(nhwc(a, g), w.float().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), None, padding=1)
    xr = xr + bias.view(1, -1, 1, 1)
    if resid:
        xr = xr + nhwc(r, g)
    assert rel(nhwc(outs[1][0], g), xr) < 1e-2


def test_groupnorm_x_from_rejects_mismatch(O):
    """x_from whose output is not exactly x (here: a different buffer) is refused, not guessed."""
    import ctypes as C
    from encdiff_amd import _lib as L
    from encdiff_amd.ops import Geom, _conv_geom
    g = Geom(8, 4, 4)
    a = bf(g.pixels, 64)
    w = bf(64, 9 * 64)
    x = torch.empty(g.pixels, 64, device=dev, dtype=torch.bfloat16)
    other = torch.empty_like(x)
    fold = O.SPLIT_FOLD
    O.SPLIT_FOLD = 0
    try:
        args = O.gemm_args(g.pixels, 64, 9 * 64, a, 64, w, 9 * 64, x, 64, a_mode=L.OPA_IM2COL,
                           conv=_conv_geom(g, 64, L.RESAMPLE_NONE, a), split_k=4)
    finally:
        O.SPLIT_FOLD = fold
    planned = C.c_int(0)
    O.check(O.lib.encdiff_gemm_ex(C.byref(args), 1, C.byref(planned), O._s()), "gemm_ex")
    assert planned.value == 1
    y = torch.empty_like(x)
    st = torch.empty(8 * 64, device=dev)
    with pytest.raises(RuntimeError):
        O.groupnorm_fwd(other, g, torch.ones(64, device=dev), torch.zeros(64, device=dev), y, st, 1e-5, True,
                        x_from=args)
    O.finalize(args)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,C,resid", [(4096, 64, True), (1024, 128, False), (8192, 128, True), (128, 256, True),
                                        (32, 256, False), (2048, 256, True)])
def test_linear_layernorm_fused(O, M, C, resid):
    """LayerNorm in the producing GEMM's epilogue (attention.py norm1/2/3 after proj_in /
    to_out) vs the separate LayerNorm kernel: same GEMM output bitwise, normalised rows and
    (mean, rstd) within fp32 summation-order noise, and torch fp32 within bf16 tolerance.
    C = 256 takes the separate LayerNorm launch in both arms (a 64x256 tile spanning the row measured
    slower: DDIM B=8 703 -> 653 steps/s), so its GEMM output is held to the torch fp32
    product within bf16 rounding."""
    torch.manual_seed(13)
    x = bf(M, C)
    w = bf(C, C, scale=C ** -0.5)
    b = torch.randn(C, device=dev) * 0.1
    r = bf(M, C) if resid else None
    gam = torch.randn(C, device=dev)
    bet = torch.randn(C, device=dev)
    res = []
    for fused in (True, False):
        O.LN_FUSED = fused
        try:
            out = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
            y = torch.empty_like(out)
            st = torch.empty(M, 2, device=dev)
            O.linear_fwd_ln(x, w, out, gam, bet, y, st, 1e-5, bias=b, resid=r)
        finally:
            O.LN_FUSED = True
        res.append((out, y, st))
    if C <= 128:
        assert torch.equal(res[0][0], res[1][0])
        assert rel(res[0][2], res[1][2]) < 1e-5
        assert (res[0][1].float() - res[1][1].float()).abs().max().item() < 0.05
    else:
        prod = x.float() @ w.float().t() + b + (r.float() if r is not None else 0.)
        assert rel(res[0][0], prod) < 1e-2 and rel(res[1][0], prod) < 1e-2
        st_ref = torch.stack([res[0][0].float().mean(1), 1 / (res[0][0].float().var(1, unbiased=False) + 1e-5).sqrt()], 1)
        assert rel(res[0][2], st_ref) < 1e-4
    ref = F.layer_norm(res[0][0].float(), (C,), gam, bet, 1e-5)
    assert rel(res[0][1], ref) < 1e-2


@pytest.mark.parametrize("B,heads,sq,dh", [(2, 1, 1024, 128), (2, 1, 4096, 128), (2, 2, 2048, 64)])
def test_attention_fwd_streamed_kv(O, B, heads, sq, dh):
    """Heads whose K / V exceed one workgroup's LDS (the VQ AttnBlock of configs[4]'s 128x128
    first stage: 1024 tokens, dh 128) stream K / V through LDS in chunks with the query tiles
    split over workgroups; forward vs torch fp32 softmax attention."""
    torch.manual_seed(8)
    C = heads * dh
    qkv = bf(B * sq, 3 * C)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    o = torch.empty(B * sq, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B * heads, sq, device=dev)
    O.attention_fwd(q, k, v, o, lse, B, heads, sq, sq, dh)

    def split(t):
        return t.float().reshape(B, sq, heads, dh).permute(0, 2, 1, 3).reshape(B * heads, sq, dh)
    s = split(q) @ split(k).transpose(1, 2) * dh ** -0.5
    ref = (s.softmax(-1) @ split(v)).reshape(B, heads, sq, dh).permute(0, 2, 1, 3).reshape(B * sq, C)
    assert rel(o, ref) < 1e-2
    assert rel(lse, torch.logsumexp(s, -1)) < 1e-4


@pytest.mark.parametrize("dq,dc,heads,dh,sq,sk", [(64, 320, 8, 8, 256, 20), (128, 128, 4, 32, 64, 64),
                                                 (60, 20, 4, 16, 64, 20), (64, 12, 8, 8, 64, 20)])
def test_cross_attention_module(O, dq, dc, heads, dh, sq, sk):
    """The standalone CrossAttention module (attention.py:152-193): q / k / v / out on encdiff::linear (GEMM
    engine), MFMA attention, to_out -- forward and the gradients of x, context and the projection
    weights vs a torch fp32 reference on the same bf16-rounded operands.  Widths that are not
    multiples of 8 (query_dim 60, context_dim 20 / 12) run zero-padded on the same engine."""
    from encdiff_amd.ldm.modules.attention import CrossAttention
    torch.manual_seed(21)
    m = CrossAttention(dq, context_dim=dc, heads=heads, dim_head=dh).cuda()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    x = (torch.randn(2, sq, dq, device=dev)).to(torch.bfloat16).float().requires_grad_(True)
    c = (torch.randn(2, sk, dc, device=dev)).to(torch.bfloat16).float().requires_grad_(True)
    out = m(x, c)
    g = torch.randn_like(out)
    out.backward(g)
    got = [out.detach(), x.grad, c.grad, m.to_q.weight.grad, m.to_k.weight.grad, m.to_v.weight.grad]
    xr, cr = x.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
    wq, wk, wv = (t.weight.detach().clone().requires_grad_(True) for t in (m.to_q, m.to_k, m.to_v))

    def split(t):
        return t.view(t.shape[0], t.shape[1], heads, dh).permute(0, 2, 1, 3)
    q, k, v = split(xr @ wq.t()), split(cr @ wk.t()), split(cr @ wv.t())
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v
    ref = m.to_out(a.permute(0, 2, 1, 3).reshape(2, sq, heads * dh).to(torch.bfloat16).float())
    ref.backward(g)
    want = [ref.detach(), xr.grad, cr.grad, wq.grad, wk.grad, wv.grad]
    for name, a_, b_ in zip(("out", "dx", "dcontext", "dWq", "dWk", "dWv"), got, want):
        r = rel(a_, b_)
        print(name, r)
        assert r < 3e-2, (name, r)


@pytest.mark.parametrize("M,K,N,resid", [(128, 256, 256, False), (2048, 256, 768, True), (100, 512, 256, False),
                                         (512, 512, 128, True)])
def test_linear_layernorm_in_staging(O, M, K, N, resid):
    """out = LayerNorm(x) w^T + b (+ r) with the LayerNorm applied to the staged A tiles
    (EncdiffGemmArgs.lna_*, row statistics reduced per workgroup): vs torch fp32, and vs the
    LayerNorm launch + plain GEMM it replaces at inference (c > 128 transformer blocks)."""
    torch.manual_seed(41)
    x = (torch.randn(M, K, device=dev) * 1.5 + 0.3).to(torch.bfloat16)
    w = bf(N, K, scale=K ** -0.5)
    b = torch.randn(N, device=dev) * 0.1
    g = 1 + 0.1 * torch.randn(K, device=dev)
    be = 0.1 * torch.randn(K, device=dev)
    r = bf(M, N) if resid else None
    out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    O.linear_fwd(x, w, out, bias=b, resid=r, ln_in=(g, be, 1e-5))
    ref = F.layer_norm(x.float(), (K,), g, be, 1e-5) @ w.float().t() + b
    if resid:
        ref = ref + r.float()
    assert rel(out, ref) < 1e-2
    n = torch.empty_like(x)
    st = torch.empty(M, 2, device=dev)
    O.layernorm_fwd(x, g, be, n, st, 1e-5)
    two = torch.empty_like(out)
    O.linear_fwd(n, w, two, bias=b, resid=r)
    assert rel(out, two.float()) < 1e-2
