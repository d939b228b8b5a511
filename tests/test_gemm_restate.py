"""CPU checks of tests/gemm_restate.py, the reference of tests/test_gpu_gemm.py.  With integer
data in fp64 the restatement must EQUAL F.conv2d (every resample expressed as test_gpu_ops.py's
test_conv3x3 / test_conv_halo_tiles / test_conv4x4s2 express it) and autograd's input / weight
gradients of the same convs and of linear layers, so that a wrong reference cannot make a wrong
kernel pass.  Operands sit as strided views inside NaN-filled buffers: the restatement reads only
the logical operand.  The copies of the launch arithmetic are held against the library itself --
encdiff_gemm_check / encdiff_gemm_tile_shape, host-only queries that need no GPU, and the planner
functions that ask them (ops.halo_fits, ops.wg3_split, ops.wgl_split) -- where they overlap, and
against values worked out by hand."""
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


WS = 1 << 12    # fake split-K workspace address (aligned; encdiff_gemm_check dereferences nothing)
PTR = 1 << 20   # fake operand address


def lib_check(tile, split, M, N, K, a_mode, b_mode, c_mode, conv=None, *, lda=0, ldb=0, ldc=0, conv_cout=0,
              pa=None, pb=None, pc=None, ws=WS, **kw):
    """encdiff_gemm_check (the validation encdiff_gemm runs before it launches, host arithmetic only)
    on a problem with null or fake pointers: (return code, tile the launch would run)."""
    import ctypes as C
    import encdiff_amd._lib as L
    cg = L.ConvGeom() if conv is None else L.ConvGeom(batch=conv.batch, h=conv.h, w=conv.w, cin=conv.cin,
                                                      resample=conv.resample, ld_src=conv.ld_src)
    args = L.GemmArgs(M=M, N=N, K=K, a_mode=a_mode, b_mode=b_mode, c_mode=c_mode, a=pa, lda=lda, b=pb, ldb=ldb, c=pc,
                      ldc=ldc, conv=cg, conv_cout=conv_cout, alpha=1.0, split_k=split, tile=tile,
                      workspace=ws if split > 1 else None, **kw)
    t = C.c_int(0)
    rc = L.lib.encdiff_gemm_check(C.byref(args), C.byref(t))
    return rc, t.value


def lib_halo(tile, b, h, w, cin, rs, split=1, b_mode=G.OPB_ROWK, c_mode=G.OUT_BF16):
    T = G.taps(rs)[0]
    rc, _ = lib_check(tile, split, b * h * w, 64, T * cin, G.OPA_IM2COL, b_mode, c_mode, G.Conv(b, h, w, cin, rs, cin),
                      ldb=T * cin, ldc=64, conv_cout=cin)
    return rc == 0


def test_halo_copy_agrees_with_the_host_mirror():
    """Halo-tile eligibility: the library's launch validation (encdiff_gemm_check) and ops.halo_fits,
    which asks it, against this file's restatement G.halo_ok."""
    from encdiff_amd import ops as O
    assert O.HALO_TILES == G.HALO_TILES
    n = 0
    for tile in list(G.HALO_TILES) + [4, 24]:
        for b, h, w in ((64, 2, 2), (16, 4, 4), (4, 8, 8), (2, 16, 16), (1, 32, 32), (2, 64, 64), (3, 4, 8), (2, 6, 6)):
            for cin in (8, 12, 24, 64, 128, 192, 256, 512):
                for rs in (0, 1, 2, 3, 4, 5):
                    for split in (1, 2, 4):
                        for bm in (G.OPB_ROWK, G.OPB_CONV_DGRAD):
                            for cm in (G.OUT_BF16, G.OUT_F32_ATOMIC):
                                want = G.halo_ok(tile, b, h, w, cin, rs, split, b_mode=bm, c_mode=cm)
                                case = (tile, b, h, w, cin, rs, split, bm, cm)
                                assert O.halo_fits(tile, b, h, w, cin, rs, split, b_mode=bm, c_mode=cm) == want, case
                                if tile != 4:  # a ring tile: launches, but is no halo tile
                                    assert lib_halo(tile, b, h, w, cin, rs, split, bm, cm) == want, case
                                    n += 1
                        assert O.halo_fits(tile, b, h, w, cin, rs, split) == G.halo_ok(tile, b, h, w, cin, rs, split)
    assert n > 40000, n
    # the LDS limit, tile by tile: the widest window the restatement lets in is accepted, 8 more
    # source channels are refused
    for tile in G.HALO_TILES:
        for geom in ((2, 16, 16), (1, 32, 32)):
            fit = [cin for cin in range(8, 4097, 8) if G.halo_ok(tile, *geom, cin, G.NONE)]
            if fit and max(fit) < 4096:
                break
        assert fit and max(fit) < 4096, (tile, "no LDS boundary below cin = 4096")
        top = max(fit)
        assert not G.halo_ok(tile, *geom, top + 8, G.NONE)
        assert lib_halo(tile, *geom, top, G.NONE) and O.halo_fits(tile, *geom, top, G.NONE), (tile, geom, top)
        assert not lib_halo(tile, *geom, top + 8, G.NONE) and not O.halo_fits(tile, *geom, top + 8, G.NONE), (tile, top)


def lib_wg3(tile, b, h, cout, cin, rs, lda, c_mode, split, ldc=None, **ptrs):
    rc, _ = lib_check(tile, split, cout, 9 * cin, b * h * h, G.OPA_ROWM, G.OPB_IM2COL, c_mode,
                      G.Conv(b, h, h, cin, rs, cin), lda=lda, ldc=9 * cin if ldc is None else ldc, **ptrs)
    return rc == 0


def lib_wgl(M, N, K, lda, ldb, c_mode, split, ldc=None, **ptrs):
    rc, _ = lib_check(36, split, M, N, K, G.OPA_ROWM, G.OPB_ROWN, c_mode, lda=lda, ldb=ldb,
                      ldc=N if ldc is None else ldc, **ptrs)
    return rc == 0


def test_wg_copies_agree_with_the_host_mirrors():
    """ops.wg3_split / ops.wgl_split return a split the kernels accept (or None where no split
    is eligible), and the library's own check of tiles 32-34 / 36 accepts exactly the explicit
    splits the copies of the device-side checks accept."""
    from encdiff_amd import ops as O
    n3 = nl = 0
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
                            for split in (1, 2, 3, 4, 8):
                                want = G.wg3_ok(tile, b, h, h, cout, cin, rs, ld, cin, G.OUT_F32_ACCUM, split)
                                assert lib_wg3(tile, b, h, cout, cin, rs, ld, G.OUT_F32_ACCUM, split) == want, \
                                    (tile, b, h, cout, cin, rs, ld, split)
                                n3 += 1
    for M in (64, 128, 72):
        for N in (64, 96, 128):
            for K in (128, 256, 512, 768, 1000):
                for ld in (0, 4):
                    sp = O.wgl_split(M, N, K, M + ld, N, G.OUT_F32_ACCUM)
                    if sp is not None:
                        assert G.wgl_ok(M, N, K, M + ld, N, G.OUT_F32_ACCUM, sp)
                    else:  # the policy also declines K % 256 != 0 and plans without two stages per wave
                        assert (not G.wgl_ok(M, N, K, M + ld, N, G.OUT_F32_ACCUM, 1)) or K % 256 or K < 256
                    for split in (1, 2, 3, 4, 6):
                        want = G.wgl_ok(M, N, K, M + ld, N, G.OUT_F32_ACCUM, split)
                        assert lib_wgl(M, N, K, M + ld, N, G.OUT_F32_ACCUM, split) == want, (M, N, K, ld, split)
                        nl += 1
    assert n3 > 10000 and nl > 400
    assert not G.wgl_ok(64, 64, 256, 64, 64, G.OUT_BF16, 1) and not G.wgl_ok(64, 64, 768, 64, 64, G.OUT_F32, 4)
    assert G.wgl_ok(64, 64, 768, 64, 64, G.OUT_F32, 3)
    # float4 epilogue stores: with one split C itself (ldc % 4, 16-byte aligned), else the slabs;
    # A and B always 16-byte aligned
    for split in (1, 2):
        for ldc in (9 * 16, 9 * 16 + 2):
            for bad in (None, "pa", "pb", "pc", "ws"):
                p = dict(pa=PTR, pb=2 * PTR, pc=3 * PTR, ws=WS)
                if bad:
                    p[bad] += 8
                seen = (p["pa"], p["pb"], p["pc"] if split == 1 else p["ws"])
                want = G.wg3_ok(32, 8, 16, 16, 32, 16, 0, 32, 16, G.OUT_F32_ACCUM, split, ldc=ldc, ptrs=seen)
                assert want == (not (bad in ("pa", "pb", "pc" if split == 1 else "ws") or (split == 1 and ldc % 4)))
                assert lib_wg3(32, 8, 16, 32, 16, 0, 32, G.OUT_F32_ACCUM, split, ldc=ldc, **p) == want, (split, ldc, bad)
                want = G.wgl_ok(64, 64, 512, 64, 64, G.OUT_F32_ACCUM, split, ldc=ldc, ptrs=seen)
                assert lib_wgl(64, 64, 512, 64, 64, G.OUT_F32_ACCUM, split, ldc=ldc, **p) == want, (split, ldc, bad)


REFUSALS = [  # (refused, M, N, K, a_mode, b_mode, c_mode, conv, bias_grad / gn_stats)
    (False, 512, 16, 32, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_BF16, G.Conv(32, 4, 4, 8, G.K4S2_TP, 8), {}),
    (True, 512, 16, 32, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_F32_ATOMIC, G.Conv(32, 4, 4, 8, G.K4S2_TP, 8), {}),
    (True, 512, 16, 32, G.OPA_IM2COL, G.OPB_ROWK, G.OUT_BF16, G.Conv(32, 4, 4, 8, G.K4S2_TP, 8), {}),
    (True, 512, 16, 128, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_BF16, G.Conv(32, 4, 4, 8, G.K4S2_TP, 8), {}),  # K != 4 cin
    (True, 256, 16, 32, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_BF16, G.Conv(16, 4, 4, 8, G.K4S2_TP, 8), {}),
    (True, 64, 16, 72, G.OPA_IM2COL, G.OPB_ROWK, G.OUT_BF16, G.Conv(1, 8, 8, 8, G.DOWN2, 8), {}),
    (True, 64, 16, 36, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, None, {}),                                          # K % 8
    (True, 60, 16, 64, G.OPA_ROWM, G.OPB_ROWN, G.OUT_F32, None, {}),                                           # M % 8
    (True, 64, 20, 64, G.OPA_ROWK, G.OPB_ROWN, G.OUT_BF16, None, {}),                                          # N % 8
    (False, 64, 20, 64, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, None, {}),
    (True, 64, 16, 64, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, None, dict(bias_grad=True)),
    (True, 72, 16, 64, G.OPA_ROWK, G.OPB_ROWK, G.OUT_BF16, None, dict(gn_stats=True)),
]


def test_refusal_copy_by_hand():
    """The tile-independent refusals, by hand; the library's check (tile 4) agrees with the copy."""
    for want, M, N, K, am, bm, cm, cv, kw in REFUSALS:
        assert G.gemm_refused(M, N, K, am, bm, cm, cv, **kw) == want
        ptrs = dict(bias_grad=PTR) if kw.get("bias_grad") else (dict(gn_stats=PTR, ld_gn_stats=N) if kw else {})
        cout = K // G.taps(cv.resample)[0] if bm == G.OPB_CONV_DGRAD else 0
        rc, tile = lib_check(4, 1, M, N, K, am, bm, cm, cv, lda=K, ldb=max(K, N), ldc=N, conv_cout=cout, **ptrs)
        assert (rc != 0) == want and (want or tile == 4), (M, N, K, am, bm, cm, rc, tile)


def test_tile_shapes_come_from_the_library():
    """encdiff_gemm_tile_shape: the ring and halo tiles' (BM, BN, KB, ring depth); every other id --
    auto, the gaps, the WG3 / WGL kernel ids -- is no tile shape."""
    import ctypes as C
    import encdiff_amd._lib as L
    from encdiff_amd import ops as O

    def shape(tile):
        v = [C.c_int(-1) for _ in range(4)]
        rc = L.lib.encdiff_gemm_tile_shape(tile, *(C.byref(x) for x in v))
        return rc, tuple(x.value for x in v)
    for tile in list(G.RING_TILES) + list(G.HALO_TILES):
        assert shape(tile) == (0, G.tile_shape(tile)), tile
    for tile in [0] + list(range(11, 16)) + [24] + list(range(32, 37)) + [-1, 1 << 20]:
        assert shape(tile) == (-3, (-1,) * 4), tile   # ENCDIFF_ERR_UNSUPPORTED, nothing written
    assert L.lib.encdiff_gemm_tile_shape(19, None, None, None, None) == 0
    assert O.HALO_TILES == G.HALO_TILES
    assert lib_check(0, 1, 64, 64, 64, 0, 0, 0, lda=64, ldb=64, ldc=64) == (0, 4)        # the default the launch picks
    assert lib_check(0, 1, 4096, 4096, 64, 0, 0, 0, lda=64, ldb=64, ldc=4096) == (0, 1)
    assert L.lib.encdiff_gemm_check(None, None) == -1


def test_measured_table_is_valid_where_it_was_measured():
    """Every entry of the measured tile table, at its own geometry (w = h; the batch from M for an
    im2col A, from K for an im2col B), is a plan the library accepts: keys carry (M, N, K, h), so at
    another batch, stride or alignment ops.gemm_args asks again (and falls back to the generic plan)."""
    import json
    import os
    import encdiff_amd
    table = json.load(open(os.path.join(os.path.dirname(encdiff_amd.__file__), "gemm_tiles.json")))
    n = geglu = 0
    for key, v in table.items():
        if not isinstance(v, list):   # "wg3,..." keys: a measured split alone
            continue
        parts = key.split(",")
        am, bm, cm, M, N, K = map(int, parts[:6])
        rs = h = 0
        for p in parts[6:]:
            rs, h = (int(p[1:]), h) if p[0] == "r" else (rs, int(p[1:]))
        tile, split = int(v[0]), int(v[1])
        conv, cout, T = None, 0, G.taps(rs)[0]
        if am == G.OPA_IM2COL or bm == G.OPB_IM2COL:
            if not h:
                continue
            batch, cin = (M // (h * h), K // T) if am == G.OPA_IM2COL else (K // (h * h), N // T)
            conv = G.Conv(batch, h, h, cin, rs, cin)
        ldb = {G.OPB_ROWK: K, G.OPB_ROWN: N, G.OPB_IM2COL: 0}.get(bm)
        if bm == G.OPB_CONV_DGRAD:  # packed weights [cout][taps * N]
            cout, ldb = K // T, (16 if rs in (G.K4S2_T, G.K4S2_TP) else 9) * N
        kw = {}
        if cm in (5, 6):  # the GEGLU epilogues: y output / f input
            kw, geglu = dict(aux=PTR, ld_aux=N), geglu + 1
        rc, t = lib_check(tile, split, M, N, K, am, bm, cm, conv, lda=M if am == G.OPA_ROWM else K, ldb=ldb, ldc=N,
                          conv_cout=cout, **kw)
        assert (rc, t) == (0, tile), (key, v[:2], rc)
        n += 1
    assert n > 200 and geglu > 0


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
