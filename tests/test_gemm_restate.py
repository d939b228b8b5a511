"""CPU checks of tests/gemm_restate.py, the reference of tests/test_gpu_gemm.py.  With integer
data in fp64 the restatement must EQUAL F.conv2d (every resample expressed as test_gpu_ops.py's
test_conv3x3 / test_conv_halo_tiles / test_conv4x4s2 express it) and autograd's input / weight
gradients of the same convs and of linear layers, so that a wrong reference cannot make a wrong
kernel pass.  Operands sit as strided views inside NaN-filled buffers: the restatement reads only
the logical operand.  The copies of the launch arithmetic are held against the library's host
mirrors (ops.halo_fits, ops.wg3_split, ops.wgl_split) where they overlap, and against values
worked out by hand."""
import pytest
import torch
import torch.nn.functional as F

import gemm_restate as G

F64 = torch.float64
NAN = float("nan")


def ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def put(x, strided=True):
    """(flat, ld) of x as a column slice (offset 8, stride + 24) of a NaN-filled buffer."""
    rows, cols = x.shape
    ld, left = (cols + 24, 8) if strided else (cols, 0)
    buf = torch.full((64 + rows * ld + 64,), NAN, dtype=x.dtype)
    view = buf.as_strided((rows, cols), (ld, 1), 64 + left)
    view.copy_(x)
    return G.flat(view)


def nchw(rows, b, h, w):
    return rows.reshape(b, h, w, -1).permute(0, 3, 1, 2)


def to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def conv_ref(xin, wq, mode):
    """The forward conv the way test_gpu_ops.py states it (xin: the NCHW source)."""
    if mode == G.UP2:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    if mode == G.STRIDE2:
        return F.conv2d(F.pad(xin, (0, 1, 0, 1)), wq, stride=2)
    if mode == G.K4S2:
        return F.conv2d(xin, wq, stride=2, padding=1)
    return F.conv2d(xin, wq, padding=1)


def src_geom(b, h, w, mode):
    if mode == G.UP2:
        return b, h // 2, w // 2
    if mode in (G.STRIDE2, G.K4S2):
        return b, 2 * h, 2 * w
    return b, h, w


def test_enums_match_the_binding():
    import encdiff_amd._lib as L
    assert (L.OPA_ROWK, L.OPA_IM2COL, L.OPA_ROWM) == (G.OPA_ROWK, G.OPA_IM2COL, G.OPA_ROWM)
    assert (L.OPB_ROWK, L.OPB_ROWN, L.OPB_CONV_DGRAD, L.OPB_IM2COL) == (0, 1, 2, 3)
    assert (L.OUT_BF16, L.OUT_F32, L.OUT_F32_ATOMIC, L.OUT_F32_ATOMIC_CONVW, L.OUT_F32_ACCUM) == (0, 1, 2, 3, 4)
    assert (L.RESAMPLE_NONE, L.RESAMPLE_DOWN2, L.RESAMPLE_UP2, L.RESAMPLE_STRIDE2, L.RESAMPLE_K4S2,
            L.RESAMPLE_K4S2_T, L.RESAMPLE_K4S2_TP) == (G.NONE, G.DOWN2, G.UP2, G.STRIDE2, G.K4S2, G.K4S2_T, G.K4S2_TP)


CONV_CASES = [(b, h, w, cin, mode) for mode in (G.NONE, G.UP2, G.STRIDE2, G.K4S2)
              for (b, h, w, cin) in ((3, 2, 2, 8), (2, 4, 4, 24), (1, 8, 8, 8), (2, 4, 8, 16), (2, 3, 5, 8))
              if not (mode == G.UP2 and (h | w) & 1)]


@pytest.mark.parametrize("b,h,w,cin,mode", CONV_CASES)
def test_conv_forward_weight_gradient(b, h, w, cin, mode):
    """OPA_IM2COL x OPB_ROWK (forward, + alpha, bias, resid) and OPA_ROWM x OPB_IM2COL (weight
    gradient, channels-last and through the OUT_F32_ATOMIC_CONVW scatter, + bias_grad) equal
    F.conv2d and its autograd weight gradient exactly.  A tap order, a padding side, the nearest-up
    source pixel or the stride-2 window origin stated wrongly shows here."""
    g = torch.Generator().manual_seed(100 * mode + h * w + cin)
    T, kw = G.taps(mode)
    cout = 16
    sb, sh, sw = src_geom(b, h, w, mode)
    x = ints(g, sb * sh * sw, cin)
    wf = ints(g, cout, T * cin)
    bias, resid = ints(g, cout), ints(g, b * h * w, cout)
    wq = wf.reshape(cout, kw, kw, cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = conv_ref(nchw(x, sb, sh, sw), wq, mode)
    xa, ld_src = put(x)
    wb, ldb = put(wf)
    rr, ld_r = put(resid)
    cv = G.Conv(b, h, w, cin, mode, ld_src)
    M, N, K = b * h * w, cout, T * cin
    P = G.Problem(M, N, K, G.OPA_IM2COL, G.OPB_ROWK, G.OUT_F32, xa, ld_src, wb, ldb, conv=cv, alpha=-2.0,
                  bias=bias, resid=rr, ld_resid=ld_r)
    got = G.result(P)["c"]
    assert torch.equal(got, -2.0 * to_rows(ref) + bias + resid)
    # weight gradient: dW[co][tap*cin + ci] = sum_p dY[p][co] im2col(x)[p][tap*cin + ci]
    dy = ints(g, M, cout)
    ref.backward(nchw(dy, b, h, w))
    dw_cl = wq.grad.permute(0, 2, 3, 1).reshape(cout, T * cin)
    da, lda = put(dy)
    c0 = ints(g, cout, T * cin)
    c0f, ldc = put(c0)
    bg0 = ints(g, cout)
    W = G.Problem(cout, T * cin, M, G.OPA_ROWM, G.OPB_IM2COL, G.OUT_F32_ACCUM, da, lda, xa, ld_src, conv=cv,
                  c_in=c0f, ldc=ldc, bias_grad_in=bg0)
    r = G.result(W)
    assert torch.equal(r["c"], c0 + dw_cl)
    assert torch.equal(r["bias_grad"], bg0 + dy.sum(0))
    if T == 9:  # the scatter to the reference Conv2d layout [co][ci][3][3]
        W.c_mode, W.convw_cin = G.OUT_F32_ATOMIC_CONVW, cin
        assert torch.equal(G.result(W)["c"], c0 + wq.grad.reshape(cout, cin * 9))


@pytest.mark.parametrize("b,h,w,cout", [(3, 2, 2, 8), (2, 4, 4, 24), (1, 8, 8, 8), (2, 4, 8, 16), (2, 3, 5, 8)])
def test_conv3x3_input_gradient(b, h, w, cout):
    """OPA_IM2COL(dY) x OPB_CONV_DGRAD equals autograd's input gradient of the 3x3 conv."""
    g = torch.Generator().manual_seed(h * w + cout)
    cin = 16
    wf, dy = ints(g, cout, 9 * cin), ints(g, b * h * w, cout)
    x = torch.zeros(b, cin, h, w, dtype=F64, requires_grad=True)
    wq = wf.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    F.conv2d(x, wq, padding=1).backward(nchw(dy, b, h, w))
    da, ld = put(dy)
    wb, ldb = put(wf)
    P = G.Problem(b * h * w, cin, 9 * cout, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_F32, da, ld, wb, ldb,
                  conv=G.Conv(b, h, w, cout, G.NONE, ld), conv_cout=cout)
    assert torch.equal(G.result(P)["c"], to_rows(x.grad))


@pytest.mark.parametrize("b,h,w,cout", [(2, 2, 2, 8), (3, 4, 4, 8), (1, 8, 8, 16), (2, 4, 8, 8)])
def test_conv4x4s2_input_gradient_both_forms(b, h, w, cout):
    """K4S2_T (16 taps, 3 of 4 masked) and K4S2_TP (parity-major rows, 2x2 taps, rows written to
    their pixel) both equal autograd's input gradient of Conv2d(k4, s2, p1) -- and so each other.
    (h, w) is the gradient's grid, dY lives at (h/2, w/2)."""
    g = torch.Generator().manual_seed(7 * h + w + cout)
    cin = 8
    wf, dy = ints(g, cout, 16 * cin), ints(g, b * (h // 2) * (w // 2), cout)
    x = torch.zeros(b, cin, h, w, dtype=F64, requires_grad=True)
    wq = wf.reshape(cout, 4, 4, cin).permute(0, 3, 1, 2)
    F.conv2d(x, wq, stride=2, padding=1).backward(nchw(dy, b, h // 2, w // 2))
    da, ld = put(dy)
    wb, ldb = put(wf)
    res = []
    for mode, T in ((G.K4S2_T, 16), (G.K4S2_TP, 4)):
        P = G.Problem(b * h * w, cin, T * cout, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_F32, da, ld, wb, ldb,
                      conv=G.Conv(b, h, w, cout, mode, ld), conv_cout=cout)
        res.append(G.result(P)["c"])
        assert torch.equal(res[-1], to_rows(x.grad)), mode
    assert torch.equal(res[0], res[1])


def test_tp_rows_are_parity_major():
    """Row r of a K4S2_TP GEMM: parity q = r // (M / 4), then (b, y', x') -> pixel (b, 2y'+py, 2x'+px)."""
    cv = G.Conv(2, 4, 6, 8, G.K4S2_TP, 8)
    _, _, out, q = G.im2col_index(cv)
    M = 2 * 4 * 6
    assert sorted(out.tolist()) == list(range(M))
    assert q.tolist() == [r // (M // 4) for r in range(M)]
    r = 3 * (M // 4) + (1 * 2 + 1) * 3 + 2   # q = 3 (py = px = 1), b = 1, y' = 1, x' = 2
    assert out[r].item() == (1 * 4 + 2 * 1 + 1) * 6 + 2 * 2 + 1


def test_linear_layers():
    """ROWK x ROWK (forward), ROWK x ROWN (input gradient) and ROWM x ROWN (weight gradient +
    bias gradient) against autograd of y = x W^T, from strided operands."""
    g = torch.Generator().manual_seed(3)
    M, N, K = 21, 12, 40
    x = ints(g, M, K).requires_grad_(True)
    w = ints(g, N, K).requires_grad_(True)
    bias, dy = ints(g, N), ints(g, M, N)
    y = x @ w.t() + bias
    y.backward(dy)
    xa, ldx = put(x.detach())
    wb, ldw = put(w.detach())
    dya, ldy = put(dy)
    P = G.Problem(M, N, K, G.OPA_ROWK, G.OPB_ROWK, G.OUT_F32, xa, ldx, wb, ldw, bias=bias)
    assert torch.equal(G.result(P)["c"], y.detach())
    P = G.Problem(M, K, N, G.OPA_ROWK, G.OPB_ROWN, G.OUT_F32, dya, ldy, wb, ldw)
    assert torch.equal(G.result(P)["c"], x.grad)
    bg = ints(g, N)
    P = G.Problem(N, K, M, G.OPA_ROWM, G.OPB_ROWN, G.OUT_F32_ATOMIC, dya, ldy, xa, ldx, alpha=0.5,
                  c_in=torch.zeros(N * K, dtype=F64), ldc=K, bias_grad_in=bg)
    r = G.result(P)
    assert torch.equal(r["c"], 0.5 * w.grad) and torch.equal(r["bias_grad"], bg + dy.sum(0))


def test_gn_stats_and_exact_bound():
    g = torch.Generator().manual_seed(5)
    M, N, K = 128, 24, 16
    x, w = ints(g, M, K, lo=-1, hi=1), ints(g, N, K, lo=-1, hi=1)
    P = G.Problem(M, N, K, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, x.reshape(-1), K, w.reshape(-1), K, gn_stats=True)
    r = G.result(P)
    y = (x @ w.t()).reshape(2, 64, N)
    assert torch.equal(r["gn_stats"][0::2], y.sum(1)) and torch.equal(r["gn_stats"][1::2], (y * y).sum(1))
    assert G.exact_bound(P) == (x.abs() @ w.abs().t()).max().item()
    P.alpha = 0.5   # halves: the bound counts units of 1/2
    assert G.exact_bound(P) == 2 * (x.abs() @ w.abs().t()).max().item()


def test_issue_numbers_for_the_exact_regime():
    """Integers in [-3, 3] at K = 4608: the fp32 matmul equals fp64 bitwise, and a good share of
    the results change when rounded to bf16 (the rounding mode is exercised)."""
    g = torch.Generator().manual_seed(0)
    a, b = ints(g, 128, 4608), ints(g, 4608, 64)
    c64 = a @ b
    assert torch.equal((a.float() @ b.float()).double(), c64)
    assert (a.abs() @ b.abs()).max().item() < 2 ** 24
    changed = (c64.float().to(torch.bfloat16).double() != c64).double().mean().item()
    assert changed > 0.05, changed


# ------------------------------------------------------------------ launch-path arithmetic
def test_split_ktiles_by_hand():
    assert G.split_ktiles(5 * 64, 64, 4) == [2, 2, 1, 0]          # the empty split of the issue's example
    assert G.split_ktiles(6 * 64, 64, 3) == [2, 2, 2]
    assert G.split_ktiles(5 * 64 - 8, 64, 2) == [3, 2]
    assert G.split_ktiles(5 * 64, 64, 12) == [1] * 5 + [0] * 7
    assert G.split_ktiles(3 * 128 + 8, 128, 1) == [4]
    assert G.halo_split_ktiles(256, G.NONE, 2) == [18, 18] and G.halo_split_ktiles(256, G.K4S2, 4) == [16] * 4
    assert G.fin_zgroups(8) == 1 and G.fin_zgroups(9) == 4
    assert G.fin_vec(20, 0) and not G.fin_vec(22, 0) and not G.fin_vec(20, 8)
    assert G.epilogue_vec(64, 64, 0) and not G.epilogue_vec(20, 20, 0) and not G.epilogue_vec(64, 68, 0)
    assert not G.epilogue_vec(64, 64, 8) and not G.epilogue_vec(64, 64, 0, bias_ptr=4)
    assert not G.epilogue_vec(64, 64, 0, resid_ptr=0, ld_resid=68)
    assert G.epilogue_vec(64, 64, 0, resid_ptr=32, ld_resid=72)
    assert G.b_pix(4, 4) and G.b_pix(8, 8) and G.b_pix(16, 16) and not G.b_pix(6, 6) and not G.b_pix(12, 4)
    assert G.tile_shape(9) == (64, 64, 64, 6) and G.tile_shape(8) == (64, 128, 128, 2) and G.tile_shape(19) == (256, 32, 64, 3)


def test_halo_copy_agrees_with_the_host_mirror():
    from encdiff_amd import ops as O
    assert O.HALO_TILES == G.HALO_TILES and O.HALO_LDS_MAX == G.HALO_LDS_MAX
    n = 0
    for tile in list(G.HALO_TILES) + [4, 24]:
        for b, h, w in ((64, 2, 2), (16, 4, 4), (4, 8, 8), (2, 16, 16), (1, 32, 32), (2, 64, 64), (3, 4, 8), (2, 6, 6)):
            for cin in (8, 12, 24, 64, 128, 192, 256, 512):
                for rs in (0, 1, 2, 3, 4, 5):
                    for split in (1, 2, 4):
                        assert O.halo_fits(tile, b, h, w, cin, rs, split) == G.halo_ok(tile, b, h, w, cin, rs, split), \
                            (tile, b, h, w, cin, rs, split)
                        n += 1
    assert n > 1000


def test_wg_copies_agree_with_the_host_mirrors():
    """ops.wg3_split / ops.wgl_split return a split the kernels accept (or None where no split
    is eligible): the copies of the device-side checks must accept exactly those."""
    from encdiff_amd import ops as O
    for tile in (32, 33, 34):
        for b in (1, 2, 4, 6, 8, 16, 32, 128):
            for h in (2, 4, 8, 16, 32):
                for cout, cin in ((32, 16), (64, 48), (48, 16), (32, 24)):
                    for rs in (0, 2, 3):
                        for ld in (cout, cout + 4):
                            sp = O.wg3_split(b, h, h, cout, cin, rs, ld, cin, G.OUT_F32_ACCUM, tile=tile)
                            any_ok = G.wg3_ok(tile, b, h, h, cout, cin, rs, ld, cin, G.OUT_F32_ACCUM, 1)
                            assert (sp is not None) == any_ok, (tile, b, h, cout, cin, rs, ld)
                            if sp is not None:
                                assert G.wg3_ok(tile, b, h, h, cout, cin, rs, ld, cin, G.OUT_F32_ACCUM, sp)
    for M in (64, 128, 72):
        for N in (64, 96, 128):
            for K in (128, 256, 512, 768, 1000):
                for ld in (0, 4):
                    sp = O.wgl_split(M, N, K, M + ld, N, G.OUT_F32_ACCUM)
                    if sp is not None:
                        assert G.wgl_ok(M, N, K, M + ld, N, G.OUT_F32_ACCUM, sp)
                    else:  # the mirror also declines K % 256 != 0 and plans without two stages per wave
                        assert (not G.wgl_ok(M, N, K, M + ld, N, G.OUT_F32_ACCUM, 1)) or K % 256 or K < 256
    assert not G.wgl_ok(64, 64, 256, 64, 64, G.OUT_BF16, 1) and not G.wgl_ok(64, 64, 768, 64, 64, G.OUT_F32, 4)
    assert G.wgl_ok(64, 64, 768, 64, 64, G.OUT_F32, 3)


def test_refusal_copy_by_hand():
    cv = G.Conv(32, 4, 4, 8, G.K4S2_TP, 8)
    assert not G.gemm_refused(512, 16, 32, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_BF16, cv)
    assert G.gemm_refused(512, 16, 32, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_F32_ATOMIC, cv)
    assert G.gemm_refused(512, 16, 32, G.OPA_IM2COL, G.OPB_ROWK, G.OUT_BF16, cv)
    assert G.gemm_refused(512, 16, 128, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_BF16, cv)            # K != 4 cin
    assert G.gemm_refused(256, 16, 32, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_BF16, G.Conv(16, 4, 4, 8, G.K4S2_TP, 8))
    assert G.gemm_refused(64, 16, 72, G.OPA_IM2COL, G.OPB_ROWK, G.OUT_BF16, G.Conv(1, 8, 8, 8, G.DOWN2, 8))
    assert G.gemm_refused(64, 16, 36, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16)                            # K % 8
    assert G.gemm_refused(60, 16, 64, G.OPA_ROWM, G.OPB_ROWN, G.OUT_F32)                             # M % 8
    assert G.gemm_refused(64, 20, 64, G.OPA_ROWK, G.OPB_ROWN, G.OUT_BF16)                            # N % 8
    assert not G.gemm_refused(64, 20, 64, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16)
    assert G.gemm_refused(64, 16, 64, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, bias_grad=True)
    assert G.gemm_refused(72, 16, 64, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, gn_stats=True)


def test_pair_route_by_hand():
    lin_w, lin_d = (G.OPA_ROWM, G.OPB_ROWN), (G.OPA_ROWK, G.OPB_ROWN)
    cv_w, cv_d = (G.OPA_ROWM, G.OPB_IM2COL), (G.OPA_IM2COL, G.OPB_CONV_DGRAD)
    assert G.pair_route(lin_w, 4, lin_d, 4) == "gemm2" and G.pair_route(lin_w, 10, lin_d, 9) == "gemm2"
    assert G.pair_route(lin_w, 1, lin_d, 4) == "separate" and G.pair_route(lin_w, 4, cv_d, 4) == "separate"
    assert G.pair_route(lin_w, 36, lin_d, 4) == "wgl_pair" and G.pair_route(lin_w, 36, lin_d, 6) == "separate"
    assert G.pair_route(lin_w, 36, lin_d, 4, d_folded=True) == "separate"
    assert G.pair_route(cv_w, 32, cv_d, 16) == "wg3_pair" and G.pair_route(cv_w, 33, cv_d, 4) == "separate"
    assert G.pair_route(cv_w, 32, cv_d, 1) == "separate" and G.pair_route(cv_w, 4, cv_d, 4) == "gemm2"
    assert G.pair_finalize(True, True) == "both" and G.pair_finalize(True, True, defer_w=True) == "d"
    assert G.pair_finalize(True, False) == "w" and G.pair_finalize(False, False) is None
    assert G.halo_window(16, 2, 2) == (16, 2) and G.halo_window(19, 16, 16) == (1, 16) and G.halo_window(16, 32, 32) == (1, 2)
