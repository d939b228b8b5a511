"""Pure-torch restatement of the GEMM / implicit-im2col conv engine (csrc/gemm.hip, the GEMM of
csrc/fp32.hip), written from include/encdiff_hip.h's description of EncdiffGemmArgs -- operand
modes, resample modes, output modes, strides -- not from the kernels' loops.
tests/test_gpu_gemm.py compares the HIP kernels with it; tests/test_gemm_restate.py checks the
restatement itself on the CPU against F.conv2d and autograd.

A[M][K] and B[K][N] are built as DENSE matrices by explicit index arithmetic on the operands' flat
storage (base pointer + leading dimension, exactly what the C ABI receives), then
    C = alpha * A B (+ bias) (+ resid) (+ C_in for the accumulating / atomic modes)
is one matmul in the dtype asked for: fp64 is the reference, fp32 the "torch fp32 evaluation" of
the rounded cases.  Nothing here reads an element outside the logical operand, so an operand may
sit inside a NaN-filled buffer.

The second half copies the pure arithmetic of the launch paths a test must be able to assert
(tile shapes, k-tile counts, split ranges, the epilogue's vector condition, the finalize's
shape), as norm_restate.GnPath copies gn_slice.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

F32 = torch.float32
F64 = torch.float64
BF16 = torch.bfloat16

# include/encdiff_hip.h enums (test_gemm_restate.py checks them against encdiff_amd._lib)
OPA_ROWK, OPA_IM2COL, OPA_ROWM = 0, 1, 2
OPB_ROWK, OPB_ROWN, OPB_CONV_DGRAD, OPB_IM2COL = 0, 1, 2, 3
OUT_BF16, OUT_F32, OUT_F32_ATOMIC, OUT_F32_ATOMIC_CONVW, OUT_F32_ACCUM = 0, 1, 2, 3, 4
NONE, DOWN2, UP2, STRIDE2, K4S2, K4S2_T, K4S2_TP = 0, 1, 2, 3, 4, 5, 6


# ------------------------------------------------------------------ operands as the ABI sees them
def flat(view):
    """(flat storage from the view's first element, leading dimension) of a row-major 2-D view."""
    assert view.dim() == 2 and view.stride(1) == 1
    rows, cols = view.shape
    ld = view.stride(0)
    return view.as_strided(((rows - 1) * ld + cols,), (1,)), ld


@dataclass
class Conv:
    """EncdiffConvGeom: (h, w) is the conv input after resampling (== the output grid)."""
    batch: int
    h: int
    w: int
    cin: int
    resample: int = NONE
    ld_src: int = 0


@dataclass
class Problem:
    """The fields of EncdiffGemmArgs that define the result.  a / b / resid / c_in are FLAT
    tensors starting at the pointer the library receives."""
    M: int
    N: int
    K: int
    a_mode: int
    b_mode: int
    c_mode: int
    a: torch.Tensor
    lda: int
    b: torch.Tensor
    ldb: int
    conv: Optional[Conv] = None
    conv_cout: int = 0
    convw_cin: int = 0
    alpha: float = 1.0
    bias: Optional[torch.Tensor] = None
    resid: Optional[torch.Tensor] = None
    ld_resid: int = 0
    c_in: Optional[torch.Tensor] = None   # accumulating / atomic modes: C before the launch, flat
    ldc: int = 0
    bias_grad_in: Optional[torch.Tensor] = None  # OPA_ROWM: bias_grad before the launch ([M])
    gn_stats: bool = False


def taps(resample):
    """(taps, taps per row) of the im2col window."""
    if resample in (K4S2, K4S2_T):
        return 16, 4
    if resample == K4S2_TP:
        return 4, 2
    return 9, 3


def src_hw(cv):
    """Spatial size of the SOURCE tensor of an im2col operand."""
    if cv.resample in (UP2, K4S2_T, K4S2_TP):
        return cv.h // 2, cv.w // 2
    if cv.resample in (STRIDE2, K4S2):
        return 2 * cv.h, 2 * cv.w
    return cv.h, cv.w


def im2col_index(cv, device="cpu"):
    """For every GEMM row r and tap t of the window: (source pixel [R][T], valid [R][T],
    output pixel [R], parity class [R]).  Rows are the batch*h*w output pixels in order, except
    K4S2_TP whose rows are parity-major [q][b][y'][x'] over the half-resolution grid and go to
    output pixel (b, 2y' + py, 2x' + px), q = 2 py + px."""
    T, kw = taps(cv.resample)
    rs = cv.resample
    hs, ws = src_hw(cv)
    R = cv.batch * cv.h * cv.w
    r = torch.arange(R, device=device)
    t = torch.arange(T, device=device)
    ty, tx = (t // kw)[None, :], (t % kw)[None, :]
    if rs == K4S2_TP:
        h2, w2, q4 = cv.h // 2, cv.w // 2, R // 4
        q, rr = r // q4, r % q4
        b, y2, x2 = rr // (h2 * w2), (rr % (h2 * w2)) // w2, rr % w2
        py, px = q // 2, q % 2
        out = (b * cv.h + 2 * y2 + py) * cv.w + 2 * x2 + px
        ys = (y2 + py)[:, None] + ty - 1   # the 2x2 taps that reach this parity class
        xs = (x2 + px)[:, None] + tx - 1
        ok = (ys >= 0) & (ys < h2) & (xs >= 0) & (xs < w2)
        src = (b[:, None] * hs + ys) * ws + xs
        return src, ok, out, q
    b, y, x = r // (cv.h * cv.w), (r % (cv.h * cv.w)) // cv.w, r % cv.w
    b, y, x = b[:, None], y[:, None], x[:, None]
    if rs in (NONE, UP2):       # 3x3, pad 1, on the (h, w) grid; UP2: nearest x2 of (h/2, w/2)
        ys, xs = y + ty - 1, x + tx - 1
        ok = (ys >= 0) & (ys < cv.h) & (xs >= 0) & (xs < cv.w)
        if rs == UP2:
            ys, xs = ys // 2, xs // 2
    elif rs == STRIDE2:         # F.pad(x, (0, 1, 0, 1)) + Conv2d(k3, s2, p0) of the (2h, 2w) source
        ys, xs = 2 * y + ty, 2 * x + tx
        ok = (ys < 2 * cv.h) & (xs < 2 * cv.w)
    elif rs == K4S2:            # Conv2d(k4, s2, p1) of the (2h, 2w) source
        ys, xs = 2 * y + ty - 1, 2 * x + tx - 1
        ok = (ys >= 0) & (ys < 2 * cv.h) & (xs >= 0) & (xs < 2 * cv.w)
    elif rs == K4S2_T:          # its input gradient: dX[y] takes dY[(y + ty - 2) / 2] where that is whole
        ys, xs = y + ty - 2, x + tx - 2
        ok = (ys >= 0) & (ys < cv.h) & (xs >= 0) & (xs < cv.w) & (ys % 2 == 0) & (xs % 2 == 0)
        ys, xs = ys // 2, xs // 2
    else:
        raise ValueError(f"resample {rs} has no im2col form")
    src = (b * hs + ys) * ws + xs
    return src, ok, r, torch.zeros_like(r)


def im2col_matrix(buf, cv, dtype):
    """[R][T * cin]: element (r, t * cin + c) = source[pixel(r, t)][c], zero where the tap is padding."""
    src, ok, _, _ = im2col_index(cv, buf.device)
    c = torch.arange(cv.cin, device=buf.device)
    idx = torch.where(ok, src, torch.zeros_like(src))[:, :, None] * cv.ld_src + c
    v = buf[idx.reshape(-1)].reshape(idx.shape).to(dtype)
    v = torch.where(ok[:, :, None], v, torch.zeros((), dtype=dtype, device=buf.device))
    return v.reshape(src.shape[0], -1)


def dense_a(P, dtype=F64):
    dev = P.a.device
    if P.a_mode == OPA_ROWK:     # A[m][k] at a + m*lda + k
        idx = torch.arange(P.M, device=dev)[:, None] * P.lda + torch.arange(P.K, device=dev)[None, :]
        return P.a[idx].to(dtype)
    if P.a_mode == OPA_ROWM:     # A[m][k] at a + k*lda + m
        idx = torch.arange(P.K, device=dev)[None, :] * P.lda + torch.arange(P.M, device=dev)[:, None]
        return P.a[idx].to(dtype)
    A = im2col_matrix(P.a, P.conv, dtype)
    assert A.shape == (P.M, P.K), (A.shape, P.M, P.K)
    return A


def dgrad_weight_tap(resample, parity=0):
    """OPB_CONV_DGRAD: the packed-weight tap read by im2col tap t (the kernel flipped)."""
    T, kw = taps(resample)
    t = torch.arange(T)
    if resample == K4S2_TP:      # window tap (jy, jx) of parity (py, px) is 4x4 tap (py + 2jy, px + 2jx)
        py, px = parity // 2, parity % 2
        return 15 - (4 * (py + 2 * (t // 2)) + px + 2 * (t % 2))
    return (T - 1) - t


def dense_b(P, dtype=F64, parity=0):
    dev = P.b.device
    k = torch.arange(P.K, device=dev)[:, None]
    n = torch.arange(P.N, device=dev)[None, :]
    if P.b_mode == OPB_ROWK:     # B[k][n] at b + n*ldb + k
        return P.b[n * P.ldb + k].to(dtype)
    if P.b_mode == OPB_ROWN:     # B[k][n] at b + k*ldb + n
        return P.b[k * P.ldb + n].to(dtype)
    if P.b_mode == OPB_CONV_DGRAD:   # B[(tap, co)][ci] = Wf[co][wtap(tap)][ci], Wf rows [T][N] at stride ldb
        wt = dgrad_weight_tap(P.conv.resample, parity).to(dev)
        assert P.K == wt.numel() * P.conv_cout
        tap, co = k // P.conv_cout, k % P.conv_cout
        return P.b[co * P.ldb + wt[tap] * P.N + n].to(dtype)
    B = im2col_matrix(P.b, P.conv, dtype)   # OPB_IM2COL: B[pixel][tap*cin + c]
    assert B.shape == (P.K, P.N), (B.shape, P.K, P.N)
    return B


def product(P, dtype=F64):
    """A B in GEMM row order ([M][N]) and the output row of each GEMM row."""
    A = dense_a(P, dtype)
    if P.a_mode == OPA_IM2COL and P.conv.resample == K4S2_TP:
        _, _, out, q = im2col_index(P.conv, P.a.device)
        acc = torch.zeros(P.M, P.N, dtype=dtype, device=A.device)
        for par in range(4):
            rows = q == par
            acc[rows] = A[rows] @ dense_b(P, dtype, par)
        return acc, out, A
    return A @ dense_b(P, dtype), torch.arange(P.M, device=A.device), A


def _rows(buf, ld, rows, cols, dtype):
    idx = torch.arange(rows, device=buf.device)[:, None] * ld + torch.arange(cols, device=buf.device)[None, :]
    return buf[idx].to(dtype)


def result(P, dtype=F64):
    """dict(c = the logical output [M][N] in OUTPUT row order (CONVW: in the reference weight
    layout's column order, [M][9 * convw_cin] with column ci*9 + tap), bias_grad [M] or None,
    gn_stats [2 * M / 64][N] or None (from the bf16-rounded c))."""
    acc, out_row, A = product(P, dtype)
    v = acc * P.alpha
    if P.bias is not None:
        v = v + P.bias.to(dtype)[None, :]
    c = torch.empty_like(v)
    c[out_row] = v
    if P.c_mode == OUT_F32_ATOMIC_CONVW:   # column n = (tap, ci) -> ci*9 + tap
        n = torch.arange(P.N, device=c.device)
        dst = (n % P.convw_cin) * 9 + n // P.convw_cin
        s = torch.empty_like(c)
        s[:, dst] = c
        c = s
    if P.resid is not None:
        c = c + _rows(P.resid, P.ld_resid, P.M, P.N, dtype)
    if P.c_mode in (OUT_F32_ATOMIC, OUT_F32_ATOMIC_CONVW, OUT_F32_ACCUM):
        c = c + _rows(P.c_in, P.ldc, P.M, P.N, dtype)
    res = {"c": c, "bias_grad": None, "gn_stats": None}
    if P.bias_grad_in is not None:
        assert P.a_mode == OPA_ROWM
        res["bias_grad"] = P.bias_grad_in.to(dtype) + A.sum(1)
    if P.gn_stats:
        assert P.c_mode == OUT_BF16 and P.M % 64 == 0
        s = c.to(F32).to(BF16).to(dtype).reshape(P.M // 64, 64, P.N)
        res["gn_stats"] = torch.stack([s.sum(1), (s * s).sum(1)], dim=1).reshape(2 * (P.M // 64), P.N)
    return res


def exact_bound(P):
    """The largest |A| |B| (+ |bias| + |resid| + |C_in|) of the problem, in units of the smallest
    fraction alpha introduces: below 2^24 every partial sum in any order, the scaled sum and the
    epilogue's additions are exact in fp32."""
    Q = Problem(**{**P.__dict__})
    Q.a, Q.b, Q.alpha = P.a.abs(), P.b.abs(), 1.0
    Q.bias = None if P.bias is None else P.bias.abs()
    Q.resid = None if P.resid is None else P.resid.abs()
    Q.c_in = None if P.c_in is None else P.c_in.abs()
    Q.bias_grad_in = None if P.bias_grad_in is None else P.bias_grad_in.abs()
    Q.gn_stats = False
    r = result(Q, F64)
    m = r["c"].max().item() * max(abs(P.alpha), 1.0)
    if r["bias_grad"] is not None:
        m = max(m, r["bias_grad"].max().item())
    frac = abs(P.alpha) % 1.0
    return m / frac if frac else m


# ====================================================================== launch-path arithmetic
# tile id -> (BM, BN, KB, ring depth): EncdiffGemmArgs.tile in include/encdiff_hip.h
RING_TILES = {1: (128, 128, 64, 2), 2: (128, 64, 64, 2), 3: (64, 128, 64, 2), 4: (64, 64, 64, 2),
              5: (64, 64, 64, 4), 6: (64, 128, 64, 3), 7: (64, 64, 128, 2), 8: (64, 128, 128, 2),
              9: (64, 64, 64, 6), 10: (64, 64, 64, 8)}
HALO_TILES = {16: (64, 64), 17: (128, 64), 18: (128, 128), 19: (256, 32), 20: (128, 32), 21: (256, 64),
              22: (64, 128), 23: (64, 32)}
HALO_RING, HALO_LDS_MAX = 3, 156 * 1024


def tile_shape(tile):
    if tile in HALO_TILES:
        return HALO_TILES[tile] + (64, HALO_RING)
    return RING_TILES[tile]


def ktiles(K, KB):
    return (K + KB - 1) // KB


def split_ktiles(K, KB, split):
    """k-tiles each split runs (ring tiles): ceil(total / split) each, the last ones short or
    EMPTY (0: such a split contributes an all-zero slab)."""
    total = ktiles(K, KB)
    per = (total + split - 1) // split
    return [max(0, min(total, (z + 1) * per) - z * per) for z in range(split)]


def halo_split_ktiles(cin, resample, split):
    """Halo tiles split over source-channel slices: every split runs all taps of its slice."""
    return [taps(resample)[0] * (cin // split // 64)] * split


def k_inner(a_mode, b_mode):
    return a_mode != OPA_ROWM or b_mode == OPB_ROWK


def xcd_order(a_mode):
    """The XCD-aware tile order is on for the k-outer-A GEMMs only (the library's default)."""
    return a_mode == OPA_ROWM


def aligned16(ptr):
    return ptr % 16 == 0


def epilogue_vec(N, ldc, c_ptr, bias_ptr=None, resid_ptr=None, ld_resid=0):
    """Whether the tile epilogue writes 8-column vectors (else one element per lane).  For a
    slab launch the arguments are the slab's: ldc = N, c = workspace, no bias / resid."""
    return (N % 8 == 0 and ldc % 8 == 0 and aligned16(c_ptr) and (bias_ptr is None or aligned16(bias_ptr)) and
            (resid_ptr is None or (ld_resid % 8 == 0 and aligned16(resid_ptr))))


def ws_path(c_mode, split):
    """split-K through fp32 slabs + a combine (else: atomics, or no split)."""
    return split > 1 and c_mode in (OUT_BF16, OUT_F32, OUT_F32_ACCUM)


def fold_ok(a_mode, c_mode, split, N, ldc, c_ptr, ws_ptr, bias_ptr=None, resid_ptr=None, ld_resid=0,
            bias_grad=False, resample=NONE, counters=True):
    """Whether the splits combine in the kernel (tickets) instead of a finalize pass."""
    return (ws_path(c_mode, split) and counters and a_mode != OPA_ROWM and not bias_grad and N % 8 == 0 and
            resample != K4S2_TP and ldc % 8 == 0 and aligned16(c_ptr) and aligned16(ws_ptr) and
            (bias_ptr is None or aligned16(bias_ptr)) and
            (resid_ptr is None or (ld_resid % 8 == 0 and aligned16(resid_ptr))))


def fin_vec(N, ws_ptr):
    """The finalize reads float4 slab lanes (else one float per lane)."""
    return N % 4 == 0 and aligned16(ws_ptr)


def fin_zgroups(split):
    """<= 8 slabs: one lane sums them all; more: four z-groups whose partials are added in order."""
    return 4 if split > 8 else 1


def b_pix(h, w, KB=64):
    """OPB_IM2COL: the per-k-tile pixel decomposition without a division (else the general path)."""
    hw = h * w
    return KB % w == 0 and (hw % KB == 0 or KB % hw == 0)


def tap_uniform(channels, KB=64):
    """A k-tile of an im2col (A) / flipped-weight (B) operand lies inside one tap."""
    return channels % KB == 0


def gemm_refused(P_M, P_N, P_K, a_mode, b_mode, c_mode, conv=None, bias_grad=False, gn_stats=False, split=1):
    """The shape refusals of encdiff_gemm that do not depend on the tile."""
    if min(P_M, P_N, P_K) <= 0:
        return True
    if k_inner(a_mode, b_mode) and P_K % 8:
        return True
    if a_mode == OPA_ROWM and P_M % 8:
        return True
    if b_mode != OPB_ROWK and P_N % 8:
        return True
    im2 = a_mode == OPA_IM2COL or b_mode == OPB_IM2COL
    if im2:
        if conv.cin % 8 or conv.resample == DOWN2:
            return True
        if conv.resample == K4S2_TP:
            if a_mode != OPA_IM2COL or b_mode != OPB_CONV_DGRAD:
                return True
            if (conv.h | conv.w) & 1 or P_M != conv.batch * conv.h * conv.w or (P_M >> 2) % 128 or P_K != 4 * conv.cin:
                return True
            if c_mode in (OUT_F32_ATOMIC, OUT_F32_ATOMIC_CONVW):
                return True
    if bias_grad and a_mode != OPA_ROWM:
        return True
    if gn_stats and (c_mode != OUT_BF16 or split != 1 or P_M % 64):
        return True
    return False


def halo_ok(tile, batch, h, w, cin, resample, split=1, b_mode=OPB_ROWK, c_mode=OUT_BF16):
    """Halo-tile eligibility (include/encdiff_hip.h: implicit im2col only; the window of the
    tile's pixels + a 3-deep B ring + the epilogue tile within the LDS)."""
    if tile not in HALO_TILES or cin % 8:
        return False
    if b_mode == OPB_ROWK:
        if resample not in (NONE, UP2, STRIDE2, K4S2):
            return False
    elif b_mode != OPB_CONV_DGRAD or resample != NONE:
        return False
    if c_mode in (OUT_F32_ATOMIC, OUT_F32_ATOMIC_CONVW):
        return False
    T, kt = taps(resample)
    if split > 1 and (cin % (64 * split) or (T * cin) % 64):
        return False
    bm, bn = HALO_TILES[tile]
    hw = h * w
    if (batch * hw) % bm or bm % w or (hw % bm and bm % hw):
        return False
    if resample == UP2 and (h | w) & 1:
        return False
    s = 2 if resample in (STRIDE2, K4S2) else 1
    rows = min(h, bm // w)
    ni = bm // hw if bm > hw else 1
    npix = ni * (s * (rows - 1) + kt) * (s * (w - 1) + kt)
    chunks = (npix * (cin // 8 // split) + 255) & ~255
    return max(chunks * 16 + HALO_RING * bn * 64 * 2, bm * (bn + 4) * 4) <= HALO_LDS_MAX


def wg3_waves(tile):
    return 8 if tile == 33 else 4


def wg3_ok(tile, batch, h, w, cout, cin, resample, lda, ld_src, c_mode, split, ldc=None, ptrs=()):
    """WG3 (tiles 32-34) eligibility for a given split: chunks of whole images whose 32-pixel
    stages divide among the workgroup's waves."""
    if resample not in (NONE, UP2) or h != w or h not in (4, 8, 16):
        return False
    if cout % 32 or cin % 16 or c_mode not in (OUT_F32, OUT_F32_ACCUM):
        return False
    ni, rows = (1 if h == 16 else 2), (4 if h == 4 else 2)
    if split < 1 or batch % split or (batch // split) % ni:
        return False
    if ((batch // split // ni) * (h // rows)) % wg3_waves(tile):
        return False
    if lda % 8 or ld_src % 8 or any(p % 16 for p in ptrs):
        return False
    if split == 1 and ldc is not None and ldc % 4:
        return False
    return True


def wgl_ok(M, N, K, lda, ldb, c_mode, split, ldc=None, ptrs=()):
    """WGL (tile 36) eligibility for a given split."""
    if c_mode not in (OUT_F32, OUT_F32_ACCUM):
        return False
    if M % 64 or N % 64 or split < 1 or K % (split * 128):
        return False
    if lda % 8 or ldb % 8 or any(p % 16 for p in ptrs):
        return False
    if split == 1 and ldc is not None and ldc % 4:
        return False
    return True


def halo_window(tile, h, w):
    """(images per tile, image rows per tile) of a halo tile: BM pixels are whole images (ni > 1
    or one whole image) or `rows` whole rows of one image."""
    bm = HALO_TILES[tile][0]
    return (bm // (h * w) if bm > h * w else 1), min(h, bm // w)


def pair_route(w_modes, w_tile, d_modes, d_tile, d_folded=False):
    """The grid a paired launch (weight gradient, input gradient) runs on: "wgl_pair", "wg3_pair"
    (one grid with the input gradient's tiles), "gemm2" (gemm2_kernel), or "separate" (two
    launches).  *_modes = (a_mode, b_mode)."""
    lin = w_modes == (OPA_ROWM, OPB_ROWN) and d_modes == (OPA_ROWK, OPB_ROWN)
    conv = w_modes == (OPA_ROWM, OPB_IM2COL) and d_modes == (OPA_IM2COL, OPB_CONV_DGRAD)
    if w_tile == 36:
        ok = d_modes == (OPA_ROWK, OPB_ROWN) and not d_folded and d_tile in (1, 2, 3, 4, 5, 7)
        return "wgl_pair" if ok else "separate"
    if w_tile in (32, 33, 34):
        ok = w_tile == 32 and d_modes == (OPA_IM2COL, OPB_CONV_DGRAD) and d_tile in (4, 2, 16, 17, 22)
        return "wg3_pair" if ok else "separate"
    if (lin or conv) and w_tile in (4, 5, 7, 9, 10):
        return "gemm2"
    return "separate"


def pair_finalize(w_slabs, d_slabs, defer_w=False, defer_d=False):
    """The finalize launch behind a gemm2 pair: "both" (one launch for the two problems'
    slabs), "w", "d" or None.  *_slabs: the problem leaves split-K slabs (not folded)."""
    f1, f2 = w_slabs and not defer_w, d_slabs and not defer_d
    return "both" if f1 and f2 else ("w" if f1 else ("d" if f2 else None))
