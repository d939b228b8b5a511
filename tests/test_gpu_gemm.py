"""Per-element tests of the MFMA GEMM / implicit-im2col conv engine on the MI355X: csrc/gemm.hip
(every ring tile, the halo tiles, the WG3 / WGL weight-gradient kernels, split-K in its three
forms, the paired and grouped launches) and the fp32 GEMM of csrc/fp32.hip, against
tests/gemm_restate.py (written from include/encdiff_hip.h; checked on the CPU against F.conv2d and
autograd by tests/test_gemm_restate.py).

EXACT cases.  bf16 operands hold small integers (-3 .. 3; -1 .. 1 where a sum of squares is
checked), bias / residual / previous C are integers and alpha is a power of two, so every product
and every partial sum in ANY order is an integer below 2^24 (each case asserts
gemm_restate.exact_bound(P) < 2^24 in fp64): the fp32 accumulator is exact whatever the MFMA's
order.  fp32 outputs must equal the fp64 reference and bf16 outputs its one round-to-nearest-even,
bit for bit (`same`, elementwise_restate.same_bits after `x + 0`: the sign of a zero is not part of
the contract -- fma(alpha, 0, 0) of the split-K combine and alpha * 0 of the tile epilogue differ
in it).  There is no tolerance.  Random integers expose a permutation of taps, rows, channels or
k-chunks, a dropped k-tile, a padding tap read from the neighbouring row, with overwhelming odds.

Conventions (test_gpu_elementwise.py): every output is a view inside a sentinel-filled Guard whose
other bytes must not change; plainly stored outputs are pre-filled with NaN, accumulating ones
start from integers; every operand is placed once contiguous and once as a strided, offset view
whose surrounding bytes are NaN (a read outside the logical operand poisons the result); the
split-K workspace region of a launch is NaN beforehand and the tickets are zero before and after.
Every case pins tile= and split_k=, asserts them on the built GemmArgs and asserts the branch it
names through gemm_restate's copies of the dispatch arithmetic (`expect=`): if a heuristic changes,
the case fails instead of testing nothing.  Refusals are asserted as HipError.

ROUNDED cases (Gaussian inputs, one per operand-mode pair, per weight-gradient kernel and per fp32
pair) use the two rules of elementwise_restate.py with floor = 4 x the largest |restatement in
fp32 - fp64|; they show that accumulation is fp32 at non-integer magnitudes.
No family needed a wider floor and nothing is derived beyond the two rules.  Largest floors and
largest |out - ref| measured on the MI355X (the whole file: 319 tests in about 5 s):
  bf16 outputs (ring tiles, halo, split-K finalize / fold):  floor 7.3e-6, |out - ref| 1.6e-2 (one
    bf16 rounding of values up to ~4: inside 2^-7 |ref|)
  fp32 outputs of forwards / input gradients (K 216 .. 456):  floor 7.1e-6, |out - ref| 1.1e-6
  fp32 weight gradients: ring tiles floor 1.2e-4, |out - ref| 2.1e-5; WG3 5.3e-5 / 6.2e-6;
    WGL 1.5e-4 / 9.4e-6; their bias gradients floor 1.0e-5, |out - ref| 2.6e-6
  fp32 GEMM (fp32.hip): floor 5.3e-5, |out - ref| 1.3e-5; bias gradients 8.0e-6 / 6.6e-6

The non-linear fused stagings and epilogues (agn_*, lna_*, ln_y, OUT_BF16_GEGLU, OUT_BF16_GEGLU_BWD)
need the norm restatements and derived bounds: tests/test_gpu_gemm_fused.py holds them per element,
against tests/gemm_fused_restate.py.

Kernel branch -> test
  gemm_tile ring: tiles 1-10 x the six operand-mode pairs of launch_one, ragged M and N,
    K tail 8 / KB - 8; k-tile counts 1, D-1, D, D+1, 2D+1 on a k-inner pair (ROWK x ROWK)
    and a k-outer pair (ROWM x ROWN) for every ring depth D and stage depth KB .......... test_ring_tiles
  epilogue: vector path and each way off it (N % 8, ldc % 8, c / bias / resid misaligned,
    ld_resid % 8) x OUT_BF16 / F32 / F32_ACCUM x alpha 1 / 0.5 / -2 x bias, resid ......... test_epilogue
  OUT_F32_ATOMIC, OUT_F32_ATOMIC_CONVW (column scatter) onto a non-zero C ................. test_atomic_outputs
  bias_grad: plain +=, split-K slab (finalize), atomic ..................................... test_bias_grad_writers
  gn_stats: M = 64 / 192, ragged N, BM = 64 / 128 (a tile with one live segment) .......... test_gn_stats
  xcd_remap on (OPA_ROWM) and off, > 8 workgroups .......................................... test_xcd_order
  split-K: slabs + finalize / in-kernel combine / atomics; split divides, does not, leaves
    EMPTY splits (the nkt > 0 guard: all-zero slab); <= 8 slabs and > 8 (four z-groups);
    bf16 + bias + resid, F32, F32_ACCUM; KB = 128 and 128 x 128 tiles ...................... test_split_k
  finalize scalar path (N % 4), misaligned c (2-byte and 8-byte), fold refused -> finalize  test_split_k_unaligned
  encdiff_gemm_ex deferred slabs + encdiff_gemm_finalize ................................... test_deferred_finalize
  implicit im2col A, NONE / UP2 / STRIDE2 / K4S2: 2x2, 4x4, 8x8, 4x8 images, tiles that
    straddle images, ragged M, cin 8 / 24 / 64 / 72 (tap-uniform k-tiles or not), ld_src > cin test_im2col_forward_borders
  OPB_CONV_DGRAD with NONE / K4S2_T; K4S2_TP (parity-major rows, split-K finalize row map) . test_im2col_dgrad, test_k4s2_tp
  K4S2_TP refusals, DOWN2 refused ........................................................... test_im2col_refusals
  OPB_IM2COL: b_pix fast path (4x4, 8x8, 16x16) and general path (6x6, 12x4), NONE / UP2 ... test_im2col_wgrad_operand
  halo tiles 16-23: whole images (2x2, 4x4, ni > 1) and rows of one image (16x16, 32x32),
    cin 8 / 24 / 64 / 128 / 192 (xmsk / xsh), forward NONE / UP2 / STRIDE2 / K4S2, dgrad NONE,
    refusals as halo_fits predicts, bitwise twin of the ring tile ........................... test_halo_tiles
  halo split-K over channel slices, split 2 / 4, finalize and fold ......................... test_halo_split_k
  WG3 (tiles 32 / 33 / 34): h = 4 / 8 / 16, NONE / UP2, cout 32 / 64, cin 16 / 48, smallest
    batch, split 1 / 2, non-zero dW, bias_grad; refusals .................................... test_wg3
  WGL (tile 36): M, N in {64, 128}, K = 256 {1, 2, 3}, admitted splits; refusals ........... test_wgl
  gemm2_kernel / WG3 pair / WGL pair (the fused route pinned by gemm_restate.pair_route): both
    halves exact and bitwise two separate launches, two pairs in a row (the first finalize
    rides in the second launch), encdiff_gemm_pair with gemm_finalize2_kernel ............... test_pairs
  encdiff_gemm_pair_dx deferred input-gradient finalize + encdiff_gemm_finalize ............ test_pair_dx_deferred
  encdiff_wgrad_group_plan / _launch: linear, 3x3, a chunked problem; tickets left zero ..... test_wgrad_group_exact
  fp32 GEMM (fp32.hip): its six mode pairs, OUT_F32 / F32_ACCUM, ragged M, N, K ............. test_gemm_f32
  rounded cases ............................................................................. test_rounded, test_gemm_f32
"""
import ctypes
import functools

import pytest
import torch

import elementwise_restate as R
import gemm_restate as G
import test_gpu_elementwise as E
from test_gpu_elementwise import Guard, _gen, assert_bf16_rule, assert_f32_rule

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
LIMIT = float(2 ** 24)


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    L = ops.L
    assert (L.OPA_ROWK, L.OPA_IM2COL, L.OPA_ROWM) == (G.OPA_ROWK, G.OPA_IM2COL, G.OPA_ROWM)
    assert (L.OPB_ROWK, L.OPB_ROWN, L.OPB_CONV_DGRAD, L.OPB_IM2COL) == (0, 1, 2, 3)
    assert (L.OUT_BF16, L.OUT_F32, L.OUT_F32_ATOMIC, L.OUT_F32_ATOMIC_CONVW, L.OUT_F32_ACCUM) == (0, 1, 2, 3, 4)
    assert (L.RESAMPLE_UP2, L.RESAMPLE_STRIDE2, L.RESAMPLE_K4S2, L.RESAMPLE_K4S2_T, L.RESAMPLE_K4S2_TP) == (2, 3, 4, 5, 6)
    ops.ensure_scratch()
    yield ops
    # leave the shared scratch as the library allocates it (zeros) and drop the cached operands
    ops.flush()
    torch.cuda.synchronize()
    ops._workspace().zero_()
    _halo_inputs.cache_clear()
    torch.cuda.empty_cache()


# ====================================================================== helpers
def ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def gauss(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def put(x, strided, dtype=BF16):
    """An operand on the device: contiguous, or a strided, offset view (offset 8, stride + 24)
    whose surrounding bytes are NaN."""
    x = x.to(dtype).to(E.dev)
    if not strided:
        return x.contiguous()
    return Guard(x.shape[0], x.shape[1], dtype, strided=True, init=x, fill=NAN).view


def put_at(x, ld, left, dtype=BF16):
    """An operand at a chosen stride / first column inside a NaN-filled buffer."""
    return Guard(x.shape[0], x.shape[1], dtype, init=x.to(dtype).to(E.dev), ld=ld, left=left, fill=NAN).view


def putv(x, left=4):
    """An fp32 vector (bias) inside a NaN-filled buffer, `left` floats in (4: 16-byte aligned)."""
    return Guard(1, x.numel(), F32, init=x.reshape(1, -1).to(E.dev), left=left, ld=left + x.numel(), fill=NAN).view[0]


def same(a, b):
    """Bitwise equal once a zero's sign is dropped (x + 0)."""
    return R.same_bits(a.contiguous() + 0, b.contiguous() + 0)


def first_bad(a, b):
    bad = ((a + 0) != (b + 0)) | (a.isnan() != b.isnan())
    idx = bad.nonzero()
    return f"{idx.shape[0]} of {a.numel()} elements differ, first at {idx[:4].tolist()}: got " \
           f"{[a[tuple(i)].item() for i in idx[:4]]} want {[b[tuple(i)].item() for i in idx[:4]]}"


def tickets_zero(O):
    return int(O._counters().abs().sum()) == 0


def _launch(O, args):
    O.check(O.lib.encdiff_gemm(ctypes.byref(args), O._s()), "encdiff_gemm")


def _launch_deferred(O, args):
    planned = ctypes.c_int(0)
    O.check(O.lib.encdiff_gemm_ex(ctypes.byref(args), 1, ctypes.byref(planned), O._s()), "encdiff_gemm_ex")
    return planned.value


def problem(M, N, K, a, b, a_mode, b_mode, c_mode, conv=None, conv_cout=0, convw_cin=0, alpha=1.0, bias=None,
            resid=None, c_in=None, bias_grad_in=None, gn=False):
    """gemm_restate.Problem of device views (a / b / resid / c_in: 2-D views)."""
    fa, lda = G.flat(a)
    fb, ldb = G.flat(b)
    cv = None
    if conv is not None:
        src = a if a_mode == G.OPA_IM2COL else b
        cv = G.Conv(conv[0], conv[1], conv[2], conv[3], conv[4], src.stride(0))
    fr, ldr = G.flat(resid) if resid is not None else (None, 0)
    fc, ldc = G.flat(c_in) if c_in is not None else (None, 0)
    return G.Problem(M, N, K, a_mode, b_mode, c_mode, fa, lda, fb, ldb, conv=cv, conv_cout=conv_cout,
                     convw_cin=convw_cin, alpha=alpha, bias=bias, resid=fr, ld_resid=ldr, c_in=fc, ldc=ldc,
                     bias_grad_in=bias_grad_in, gn_stats=gn)


def path_facts(O, args, P, tile, split):
    """What the launch will do, from gemm_restate's copies of the dispatch arithmetic."""
    f = {"xcd": G.xcd_order(P.a_mode), "ws_path": G.ws_path(P.c_mode, split)}
    bias_ptr = args.bias if args.bias else None
    resid_ptr = args.resid if args.resid else None
    ws_ptr = args.workspace or 0
    rs = P.conv.resample if P.conv is not None else G.NONE
    f["folded"] = bool(args.split_counters) and G.fold_ok(
        P.a_mode, P.c_mode, split, P.N, args.ldc, args.c, ws_ptr, bias_ptr, resid_ptr, args.ld_resid,
        bias_grad=bool(args.bias_grad), resample=rs)
    if f["ws_path"]:
        f["vec"] = G.epilogue_vec(P.N, P.N, ws_ptr)
        f["fin_vec"] = None if f["folded"] else G.fin_vec(P.N, ws_ptr)
        f["zgroups"] = None if f["folded"] else G.fin_zgroups(split)
    else:
        f["vec"] = G.epilogue_vec(P.N, args.ldc, args.c, bias_ptr, resid_ptr, args.ld_resid)
        f["fin_vec"] = f["zgroups"] = None
    if tile in G.RING_TILES or tile in G.HALO_TILES:
        BM, BN, KB, D = G.tile_shape(tile)
        f["blocks"] = -(-P.M // BM) * -(-P.N // BN) * split
        if tile in G.HALO_TILES and split > 1:
            f["nkt"] = G.halo_split_ktiles(P.conv.cin, rs, split)
        else:
            f["nkt"] = G.split_ktiles(P.K, KB, split)
        if P.a_mode == G.OPA_IM2COL:
            f["a_tapk"] = G.tap_uniform(P.conv.cin, KB)
        if P.b_mode == G.OPB_CONV_DGRAD:
            f["b_tapk"] = G.tap_uniform(P.conv_cout, KB)
        if P.b_mode == G.OPB_IM2COL:
            f["b_pix"] = G.b_pix(P.conv.h, P.conv.w, KB)
    return f


def run(O, M, N, K, a, b, *, tile, split=1, fold=False, a_mode=0, b_mode=0, c_mode=0, conv=None, conv_cout=0,
        convw_cin=0, alpha=1.0, bias=None, resid=None, c_init=None, bias_grad=None, gn=False, strided_out=False,
        out_at=None, expect=None, exact=True, ref=None, defer=False, what=""):
    """One launch checked per element.  conv = (batch, h, w, cin, resample).  c_init / bias_grad:
    integer start values of an accumulating C / the bias gradient.  Returns the outputs."""
    L = O.L
    expect = expect or {}
    out_dt = BF16 if c_mode == G.OUT_BF16 else F32
    accum = c_mode in (G.OUT_F32_ATOMIC, G.OUT_F32_ATOMIC_CONVW, G.OUT_F32_ACCUM)
    assert accum == (c_init is not None), "accumulating outputs start from integers, stored ones from NaN"
    init = c_init.to(E.dev) if accum else torch.full((M, N), NAN, dtype=out_dt, device=E.dev)
    if out_at is not None:
        out = Guard(M, N, out_dt, init=init, ld=out_at[0], left=out_at[1])
    else:
        out = Guard(M, N, out_dt, strided=strided_out, init=init)
    bg = None
    if bias_grad is not None:
        bg = Guard(1, M, F32, init=bias_grad.reshape(1, M).to(E.dev))
    gs = None
    if gn:
        gs = Guard(2 * (M // 64), N, F32, strided=strided_out,
                   init=torch.full((2 * (M // 64), N), NAN, device=E.dev))
    P = problem(M, N, K, a, b, a_mode, b_mode, c_mode, conv, conv_cout, convw_cin, alpha, bias, resid,
                out.view.clone() if accum else None, None if bg is None else bg.view[0].clone(), gn)
    if ref is None:
        if exact:
            bound = G.exact_bound(P)
            assert bound < LIMIT, f"{what}: |A||B| (+ ...) = {bound} leaves the exact regime"
        ref = G.result(P, F64)
    if gn and exact:  # the squares are positive, so every partial sum stays below the total
        sq = ref["gn_stats"][1::2].max().item()
        assert sq < LIMIT and 8 * sq ** 0.5 < LIMIT, f"{what}: gn_stats sums leave the exact regime"
    cg = None
    if conv is not None:
        cg = L.ConvGeom(batch=conv[0], h=conv[1], w=conv[2], cin=conv[3], resample=conv[4], ld_src=P.conv.ld_src)
    args = O.gemm_args(M, N, K, a, a.stride(0), b, b.stride(0), out.view, out.view.stride(0), a_mode=a_mode,
                       b_mode=b_mode, c_mode=c_mode, conv=cg, conv_cout=conv_cout, convw_cin=convw_cin, alpha=alpha,
                       split_k=split, bias=bias, resid=resid, ld_resid=resid.stride(0) if resid is not None else 0,
                       bias_grad=None if bg is None else bg.view, tile=tile, gn_stats=None if gs is None else gs.view,
                       fold=fold)
    assert (args.tile, args.split_k) == (tile, split), f"{what}: plan changed to {(args.tile, args.split_k)}"
    assert bool(args.split_counters) == bool(fold), f"{what}: tickets {bool(args.split_counters)}, case needs {fold}"
    facts = path_facts(O, args, P, tile, split)
    for k, v in expect.items():
        assert facts.get(k) == v, f"{what}: dispatch changed: {k} = {facts.get(k)}, this case needs {v}"
    O.flush()
    nws = O.ws_floats(args)
    if nws:
        O._workspace()[:nws].fill_(NAN)  # slabs are plain stores: an unwritten one shows
    assert tickets_zero(O)
    if defer:
        assert _launch_deferred(O, args) == 1, f"{what}: the plan left no slabs to defer"
        torch.cuda.synchronize()
        assert R.same_bits(out.buf, out.before), f"{what}: C written before the deferred finalize"
        O.finalize(args)
    else:
        _launch(O, args)
    torch.cuda.synchronize()
    assert tickets_zero(O), f"{what}: tickets not left zero"
    for gd in (out, bg, gs):
        if gd is not None:
            gd.check()
    if not exact:
        return out, bg, ref, P
    want = ref["c"].to(F32).to(out_dt)
    assert same(out.view, want), f"{what}: C: " + first_bad(out.view.contiguous(), want)
    if bg is not None:
        wb = ref["bias_grad"].to(F32)
        assert same(bg.view[0], wb), f"{what}: bias_grad: " + first_bad(bg.view[0].contiguous(), wb)
    if gs is not None:
        wg = ref["gn_stats"].to(F32)
        assert same(gs.view, wg), f"{what}: gn_stats: " + first_bad(gs.view.contiguous(), wg)
    return out, bg, ref, P


def refused(O, M, N, K, a, b, *, tile, split=1, c_mode=G.OUT_F32, **kw):
    """The library must refuse the launch (HipError) and write nothing; encdiff_gemm_check, the
    host-only query of the same validation, must refuse the same arguments."""
    out_dt = BF16 if c_mode == G.OUT_BF16 else F32
    out = Guard(M, N, out_dt, init=torch.zeros(M, N, dtype=out_dt, device=E.dev))
    conv = kw.pop("conv", None)
    cg = None
    if conv is not None:
        src = a if kw.get("a_mode", 0) == G.OPA_IM2COL else b
        cg = O.L.ConvGeom(batch=conv[0], h=conv[1], w=conv[2], cin=conv[3], resample=conv[4], ld_src=src.stride(0))
    O.flush()
    args = O.gemm_args(M, N, K, a, a.stride(0), b, b.stride(0), out.view, N, c_mode=c_mode, conv=cg, split_k=split,
                       tile=tile, **kw)
    assert (args.tile, args.split_k) == (tile, split)
    assert O.L.lib.encdiff_gemm_check(args, None) != 0
    with pytest.raises(O.L.HipError):
        O.gemm(M, N, K, a, a.stride(0), b, b.stride(0), out.view, N, c_mode=c_mode, conv=cg, split_k=split,
               tile=tile, **kw)
    torch.cuda.synchronize()
    assert R.same_bits(out.buf, out.before)


def src_pixels(batch, h, w, resample):
    cv = G.Conv(batch, h, w, 8, resample, 8)
    hs, ws = G.src_hw(cv)
    return batch * hs * ws


# ====================================================================== 1. ring tiles
PAIRS = ["rowk_rowk", "im2col_rowk", "rowk_rown", "im2col_dgrad", "rowm_rown", "rowm_im2col"]


def _dense_K(tile):
    """K values giving 1, D-1, D, D+1, 2D+1 k-tiles, the last one partial (8 or KB - 8 columns)."""
    _, _, KB, D = G.tile_shape(tile)
    counts = sorted({1, D - 1, D, D + 1, 2 * D + 1} - {0})
    return [((n - 1) * KB + (8 if i % 2 == 0 else KB - 8), n) for i, n in enumerate(counts)]


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("tile", sorted(G.RING_TILES))
def test_ring_tiles(O, tile, pair):
    """Every LDS-ring tile on every operand-mode pair launch_one dispatches, M = BM + 24 and
    N = BN + 8 (a ragged last tile in both dimensions) and a partial last k-tile.  The dense
    pairs sweep the k-tile counts around the ring depth (prologue shorter than the ring, exactly
    the ring, one and several wraps).  Catches: a ring slot read before its DMA landed or refilled
    while still read (a wrong vmcnt / stage count shows as a wrong integer), a dropped or doubled
    k-tile, the K tail not masked, the last tile's rows / columns written one off."""
    BM, BN, KB, D = G.tile_shape(tile)
    M, N = BM + 24, BN + 8
    for strided in (False, True):
        g = _gen(100 * tile + int(strided))
        what = f"ring tile {tile} {pair} strided={int(strided)}"
        if pair == "rowk_rowk":
            for K, n in _dense_K(tile):
                a, b = put(ints(g, M, K), strided), put(ints(g, N, K), strided)
                run(O, M, N, K, a, b, tile=tile, bias=putv(ints(g, N)), strided_out=strided,
                    expect={"nkt": [n], "vec": True, "xcd": False}, what=f"{what} K={K}")
        elif pair == "rowm_rown":
            for K, n in _dense_K(tile):
                a, b = put(ints(g, K, M), strided), put(ints(g, K, N), strided)
                run(O, M, N, K, a, b, tile=tile, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32_ACCUM,
                    c_init=ints(g, M, N), bias_grad=ints(g, M), strided_out=strided,
                    expect={"nkt": [n], "xcd": True}, what=f"{what} K={K}")
        elif pair == "rowk_rown":
            K = D * KB + 8
            a, b = put(ints(g, M, K), strided), put(ints(g, K, N), strided)
            run(O, M, N, K, a, b, tile=tile, b_mode=G.OPB_ROWN, alpha=0.5, resid=put(ints(g, M, N), strided),
                strided_out=strided, expect={"nkt": [D + 1]}, what=what)
        elif pair == "im2col_rowk":
            batch, cin = M // 4, 24
            a, b = put(ints(g, batch * 4, cin), strided), put(ints(g, N, 9 * cin), strided)
            run(O, M, N, 9 * cin, a, b, tile=tile, a_mode=G.OPA_IM2COL, c_mode=G.OUT_F32, conv=(batch, 2, 2, cin, G.NONE),
                strided_out=strided, expect={"a_tapk": False, "nkt": [G.ktiles(216, KB)]}, what=what)
        elif pair == "im2col_dgrad":
            batch, cout = M // 4, 24
            a, b = put(ints(g, batch * 4, cout), strided), put(ints(g, cout, 9 * N), strided)
            run(O, M, N, 9 * cout, a, b, tile=tile, a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD, c_mode=G.OUT_F32,
                conv=(batch, 2, 2, cout, G.NONE), conv_cout=cout, strided_out=strided,
                expect={"b_tapk": False}, what=what)
        else:  # rowm_im2col: the conv weight gradient, K = pixels
            cin, batch = (8 if BN == 64 else 16), 5
            K = batch * 36
            a, b = put(ints(g, K, M), strided), put(ints(g, K, cin), strided)
            run(O, M, 9 * cin, K, a, b, tile=tile, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL, c_mode=G.OUT_F32_ACCUM,
                conv=(batch, 6, 6, cin, G.NONE), c_init=ints(g, M, 9 * cin), bias_grad=ints(g, M), strided_out=strided,
                expect={"b_pix": False, "xcd": True}, what=what)


# ====================================================================== 2. epilogue
EPI = ["vec", "plain", "n20", "n130", "ldc", "c_misaligned", "bias_misaligned", "resid_misaligned", "ld_resid"]


@pytest.mark.parametrize("variant", EPI)
def test_epilogue(O, variant):
    """The vector epilogue and each way of falling off it, for the three stored / accumulated
    output modes, alpha 1 / 0.5 / -2, with bias and residual (`plain`: without).  Catches: the
    scalar path's row / column arithmetic, bias or residual read at the wrong stride, alpha applied
    after the bias, F32_ACCUM overwriting, a vector store across the end of a ragged row."""
    M, K = 88, 72
    N = {"n20": 20, "n130": 130}.get(variant, 64)
    for i, c_mode in enumerate((G.OUT_BF16, G.OUT_F32, G.OUT_F32_ACCUM)):
        for strided in (False, True):
            g = _gen(300 + 10 * i + int(strided))
            esz = 2 if c_mode == G.OUT_BF16 else 4
            alpha = (1.0, 0.5, -2.0)[(i + int(strided)) % 3]
            a, b = put(ints(g, M, K), strided), put(ints(g, N, K), strided)
            bias = None if variant == "plain" else putv(ints(g, N))
            resid = None if variant == "plain" else put(ints(g, M, N), strided)
            out_at = None
            if variant == "ldc":
                out_at = (N + 4, 0)
            elif variant == "c_misaligned":
                out_at = (N + 8, 8 // esz)            # 8 bytes off a 16-byte boundary
            elif variant == "bias_misaligned":
                bias = putv(ints(g, N), left=1)
            elif variant == "resid_misaligned":
                resid = put_at(ints(g, M, N), N + 8, 4)
            elif variant == "ld_resid":
                resid = put_at(ints(g, M, N), N + 4, 0)
            run(O, M, N, K, a, b, tile=4, c_mode=c_mode, alpha=alpha, bias=bias, resid=resid,
                c_init=ints(g, M, N) if c_mode == G.OUT_F32_ACCUM else None, strided_out=strided, out_at=out_at,
                expect={"vec": variant in ("vec", "plain"), "nkt": [2]},
                what=f"epilogue {variant} c_mode={c_mode} strided={int(strided)} alpha={alpha}")


def test_atomic_outputs(O):
    """OUT_F32_ATOMIC (+ bias, alpha) and the OUT_F32_ATOMIC_CONVW column scatter (column
    n = (tap, ci) -> ci * 9 + tap of the reference Conv2d layout) onto a non-zero C, split 1 and 2."""
    for strided in (False, True):
        g = _gen(400 + int(strided))
        M, N, K = 88, 72, 136
        a, b = put(ints(g, M, K), strided), put(ints(g, N, K), strided)
        for split in (1, 2):
            run(O, M, N, K, a, b, tile=4, split=split, c_mode=G.OUT_F32_ATOMIC, alpha=-2.0, bias=putv(ints(g, N)),
                c_init=ints(g, M, N), strided_out=strided, expect={"ws_path": False}, what=f"atomic split {split}")
        cout, cin, batch = 40, 8, 5
        Kp = batch * 16
        dy, x = put(ints(g, Kp, cout), strided), put(ints(g, Kp, cin), strided)
        for split in (1, 2):
            run(O, cout, 9 * cin, Kp, dy, x, tile=4, split=split, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL,
                c_mode=G.OUT_F32_ATOMIC_CONVW, conv=(batch, 4, 4, cin, G.NONE), convw_cin=cin,
                c_init=ints(g, cout, 9 * cin), bias_grad=ints(g, cout), expect={"b_pix": True},
                what=f"convw split {split}")


def test_bias_grad_writers(O):
    """bias_grad[m] += sum_k A[m][k] through its three writers: plain += (one K range), a slab per
    split summed by the finalize, and atomics (atomic output modes / atomic split-K)."""
    for strided in (False, True):
        g = _gen(500 + int(strided))
        M, N, K = 88, 72, 5 * 64 - 8
        a, b = put(ints(g, K, M), strided), put(ints(g, K, N), strided)
        for c_mode, split in ((G.OUT_F32_ACCUM, 1), (G.OUT_F32_ACCUM, 2), (G.OUT_F32_ACCUM, 4), (G.OUT_F32_ATOMIC, 1),
                              (G.OUT_F32_ATOMIC, 2)):
            run(O, M, N, K, a, b, tile=4, split=split, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=c_mode,
                c_init=ints(g, M, N), bias_grad=ints(g, M), strided_out=strided,
                expect={"ws_path": c_mode == G.OUT_F32_ACCUM and split > 1, "folded": False},
                what=f"bias_grad c_mode={c_mode} split={split}")


@pytest.mark.parametrize("tile,M,N", [(4, 64, 72), (4, 192, 72), (2, 192, 72), (1, 192, 136), (3, 64, 136)])
def test_gn_stats(O, tile, M, N):
    """gn_stats: per 64-row segment and column, the sum and sum of squares of the STORED bf16
    values ({-1, 0, 1} operands: every sum of squares is an exact integer).  BM = 128 with M = 192
    leaves a tile with one live segment.  Catches a segment written to the wrong slot, the
    statistics taken before the rounding, a ragged N column dropped."""
    for strided in (False, True):
        g = _gen(600 + tile + int(strided))
        K = 24
        a, b = put(ints(g, M, K, lo=-1, hi=1), strided), put(ints(g, N, K, lo=-1, hi=1), strided)
        run(O, M, N, K, a, b, tile=tile, bias=putv(ints(g, N, lo=-1, hi=1)), gn=True, strided_out=strided,
            expect={"vec": True}, what=f"gn_stats tile {tile} {M}x{N}")
        # values that round to bf16 (|v| > 256 through the bias) with sums of squares still exact
        a, b = put(ints(g, M, 264), strided), put(ints(g, N, 264, lo=-1, hi=1), strided)
        run(O, M, N, 264, a, b, tile=tile, bias=putv(ints(g, N, lo=-250, hi=250)), gn=True, strided_out=strided,
            what=f"gn_stats rounding tile {tile}")
    a, b = put(ints(g, 72, K), False), put(ints(g, N, K), False)
    gsbuf = torch.zeros(2, N, device=E.dev)
    with pytest.raises(O.L.HipError):  # M % 64 != 0
        O.gemm(72, N, K, a, K, b, K, torch.zeros(72, N, dtype=BF16, device=E.dev), N, split_k=1, tile=tile,
               gn_stats=gsbuf)


def test_xcd_order(O):
    """The XCD-aware tile order (on for OPA_ROWM, off otherwise) on grids of 18 workgroups, not a
    multiple of 8: a remap that is not a bijection leaves a tile unwritten (NaN) or written twice."""
    for strided in (False, True):
        g = _gen(700 + int(strided))
        M = N = 192
        K = 136
        a, b = put(ints(g, K, M), strided), put(ints(g, K, N), strided)
        run(O, M, N, K, a, b, tile=4, split=2, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32,
            strided_out=strided, expect={"xcd": True, "blocks": 18}, what="xcd on")
        a, b = put(ints(g, M, K), strided), put(ints(g, N, K), strided)
        run(O, M, N, K, a, b, tile=4, split=2, c_mode=G.OUT_F32, strided_out=strided,
            expect={"xcd": False, "blocks": 18}, what="xcd off")


# ====================================================================== 3. split-K
SPLITS = {"divides": (6, 3), "ragged": (5, 2), "empty": (5, 4), "z12": (12, 12), "z12_empty": (5, 12)}


@pytest.mark.parametrize("tile", [4, 1, 7])
@pytest.mark.parametrize("name", sorted(SPLITS))
@pytest.mark.parametrize("mode", ["finalize", "fold", "atomic"])
def test_split_k(O, mode, name, tile):
    """Split-K through slabs + finalize, the in-kernel combine and atomics: a split that divides
    the k-tiles, one that does not, and splits LARGER than the k-tile count (empty splits must
    contribute an all-zero slab: the workspace is NaN beforehand), with <= 8 slabs (one lane sums
    them) and > 8 (four z-groups).  Catches: a k-tile dropped or doubled at a split boundary, an
    empty split's slab left unwritten, bias added by every split, the finalize's z-group sum
    missing a slab, the tickets left non-zero."""
    kts, split = SPLITS[name]
    BM, BN, KB, D = G.tile_shape(tile)
    M, N = BM + 24, BN + 8
    K = (kts - 1) * KB + KB - 8
    nkt = G.split_ktiles(K, KB, split)
    assert sum(nkt) == kts and (0 in nkt) == ("empty" in name)
    for strided in (False, True):
        g = _gen(800 + kts + split + int(strided))
        a, b = put(ints(g, M, K), strided), put(ints(g, N, K), strided)
        bias, resid = putv(ints(g, N)), put(ints(g, M, N), strided)
        what = f"split-K {mode} {name} tile {tile} strided={int(strided)}"
        if mode == "atomic":
            run(O, M, N, K, a, b, tile=tile, split=split, c_mode=G.OUT_F32_ATOMIC, bias=bias, c_init=ints(g, M, N),
                strided_out=strided, expect={"nkt": nkt, "ws_path": False}, what=what)
            continue
        fold = mode == "fold"
        exp = {"nkt": nkt, "ws_path": True, "folded": fold, "vec": True,
               "zgroups": None if fold else (4 if split > 8 else 1), "fin_vec": None if fold else True}
        run(O, M, N, K, a, b, tile=tile, split=split, fold=fold, alpha=0.5, bias=bias, resid=resid, strided_out=strided,
            expect=exp, what=what + " bf16")
        run(O, M, N, K, a, b, tile=tile, split=split, fold=fold, c_mode=G.OUT_F32, strided_out=strided, expect=exp,
            what=what + " f32")
        run(O, M, N, K, a, b, tile=tile, split=split, fold=fold, c_mode=G.OUT_F32_ACCUM, alpha=-2.0, bias=bias,
            c_init=ints(g, M, N), strided_out=strided, expect=exp, what=what + " f32_accum")


@pytest.mark.parametrize("variant", ["n20", "n22", "c_2byte", "c_8byte", "ldc"])
def test_split_k_unaligned(O, variant):
    """The finalize's scalar path (N % 4 != 0), its float4 path with N % 8 != 0 (N = 20), and a
    misaligned / odd-stride C: the in-kernel combine is asked for and must be declined (a finalize
    pass runs), splits 3 and 12 (one of them with empty splits)."""
    M, K = 88, 5 * 64 - 8
    N = {"n20": 20, "n22": 22}.get(variant, 72)
    out_at = {"c_2byte": (N + 8, 1), "c_8byte": (N + 8, 4), "ldc": (N + 4, 0)}.get(variant)
    for split in (3, 12):
        g = _gen(900 + split)
        a, b = put(ints(g, M, K), True), put(ints(g, N, K), True)
        exp = {"folded": False, "ws_path": True, "fin_vec": N % 4 == 0, "zgroups": 4 if split > 8 else 1,
               "vec": N % 8 == 0}
        run(O, M, N, K, a, b, tile=4, split=split, fold=True, alpha=0.5, bias=putv(ints(g, N)),
            resid=put(ints(g, M, N), True), out_at=out_at, strided_out=True, expect=exp,
            what=f"split-K unaligned {variant} split {split} bf16")
        if variant in ("n20", "n22", "ldc"):
            run(O, M, N, K, a, b, tile=4, split=split, fold=True, c_mode=G.OUT_F32_ACCUM, c_init=ints(g, M, N),
                out_at=out_at, strided_out=True, expect=exp, what=f"split-K unaligned {variant} split {split} accum")


def test_deferred_finalize(O):
    """encdiff_gemm_ex with defer_finalize: only the slabs are written (C untouched), then
    encdiff_gemm_finalize completes C -- the bf16 epilogue and an accumulating fp32 one."""
    for strided in (False, True):
        g = _gen(950 + int(strided))
        M, N, K = 88, 72, 5 * 64 - 8
        a, b = put(ints(g, M, K), strided), put(ints(g, N, K), strided)
        run(O, M, N, K, a, b, tile=4, split=4, alpha=0.5, bias=putv(ints(g, N)), resid=put(ints(g, M, N), strided),
            strided_out=strided, defer=True, expect={"folded": False, "nkt": [2, 2, 1, 0]}, what="deferred bf16")
        run(O, M, N, K, a, b, tile=4, split=3, c_mode=G.OUT_F32_ACCUM, c_init=ints(g, M, N), strided_out=strided,
            defer=True, what="deferred accum")


# ====================================================================== 4. implicit im2col, borders
IMAGES = [(2, 2, 19, 4), (4, 4, 5, 4), (8, 8, 3, 2), (4, 8, 3, 4)]  # h, w, batch, tile: ragged M, tiles straddle images


@pytest.mark.parametrize("cin", [8, 24, 64, 72])
@pytest.mark.parametrize("h,w,batch,tile", IMAGES)
@pytest.mark.parametrize("rs", [G.NONE, G.UP2, G.STRIDE2, G.K4S2])
def test_im2col_forward_borders(O, rs, h, w, batch, tile, cin):
    """The forward's implicit im2col on small images, where most output pixels sit on an edge or
    a corner and a 64-row tile holds several images.  Catches: a padding tap read from the
    neighbouring image row or the neighbouring image, the window origin of STRIDE2 / K4S2 off by
    one, the nearest-up source pixel, a k-tile that straddles two taps (cin 8 / 24 / 72) decoded
    with one tap's coordinates, the pixel stride ld_src taken for cin."""
    T = G.taps(rs)[0]
    M, N, K = batch * h * w, 40, T * cin
    BM = G.tile_shape(tile)[0]
    assert M % BM, "ragged M"
    for strided in (False, True):
        g = _gen(1000 + 100 * rs + h * w + cin + int(strided))
        x = put(ints(g, src_pixels(batch, h, w, rs), cin), strided)
        wf = put(ints(g, N, K), strided)
        kw = dict(tile=tile, a_mode=G.OPA_IM2COL, conv=(batch, h, w, cin, rs), strided_out=strided,
                  expect={"a_tapk": cin % 64 == 0}, what=f"im2col fwd rs={rs} {h}x{w} cin={cin} strided={int(strided)}")
        if strided:
            run(O, M, N, K, x, wf, bias=putv(ints(g, N)), resid=put(ints(g, M, N), True), **kw)
        else:
            run(O, M, N, K, x, wf, c_mode=G.OUT_F32, **kw)


@pytest.mark.parametrize("cout", [8, 24, 64, 72])
@pytest.mark.parametrize("h,w,batch,tile", IMAGES)
@pytest.mark.parametrize("rs", [G.NONE, G.K4S2_T])
def test_im2col_dgrad(O, rs, h, w, batch, tile, cout):
    """The input gradient: im2col of dY against the flipped weight taps (OPB_CONV_DGRAD), 3x3 and
    the 16-tap transposed k4 s2 form (3 of 4 taps masked by parity).  Catches two weight taps
    swapped, the flip taken over 9 taps for a 16-tap kernel, a parity mask on one coordinate only."""
    T = G.taps(rs)[0]
    M, N, K = batch * h * w, 40, T * cout
    for strided in (False, True):
        g = _gen(1100 + 100 * rs + h * w + cout + int(strided))
        dy = put(ints(g, src_pixels(batch, h, w, rs), cout), strided)
        wf = put(ints(g, cout, T * N), strided)
        run(O, M, N, K, dy, wf, tile=tile, a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD, c_mode=G.OUT_F32,
            conv=(batch, h, w, cout, rs), conv_cout=cout, strided_out=strided,
            expect={"a_tapk": cout % 64 == 0, "b_tapk": cout % 64 == 0},
            what=f"dgrad rs={rs} {h}x{w} cout={cout} strided={int(strided)}")


@pytest.mark.parametrize("cout", [8, 24, 64])
@pytest.mark.parametrize("h,w,batch", [(4, 4, 32), (2, 2, 128), (8, 8, 8), (4, 8, 16)])
def test_k4s2_tp(O, h, w, batch, cout):
    """K4S2_TP: rows computed parity-major with the 2x2 taps of their parity class, written to
    their pixel -- by the tile epilogue, by the finalize (split 3: slabs stay in GEMM row order)
    -- with a residual read at the OUTPUT row.  64- and 128-row tiles."""
    M, N, K = batch * h * w, 40, 4 * cout
    for strided, tile, split in ((False, 4, 1), (True, 2, 1), (True, 4, 3)):
        g = _gen(1200 + h * w + cout + int(strided) + split)
        dy = put(ints(g, src_pixels(batch, h, w, G.K4S2_TP), cout), strided)
        wf = put(ints(g, cout, 16 * N), strided)
        run(O, M, N, K, dy, wf, tile=tile, split=split, a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD,
            conv=(batch, h, w, cout, G.K4S2_TP), conv_cout=cout, alpha=0.5, resid=put(ints(g, M, N), strided),
            strided_out=strided, expect={"folded": False}, what=f"k4s2_tp {h}x{w} cout={cout} tile {tile} split {split}")


def test_im2col_refusals(O):
    """Shapes the library must refuse, in agreement with gemm_restate.gemm_refused."""
    g = _gen(1300)
    cout, N = 8, 16
    dy = put(ints(g, 2048, cout), False)
    wf = put(ints(g, 16, 16 * N), False)   # (sized for every case below, should one not be refused)
    tp = dict(a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD, conv_cout=cout)
    cases = [  # (M, K, conv, c_mode, overrides)
        (512, 32, (32, 4, 4, cout, G.K4S2_TP), G.OUT_F32_ATOMIC, {}),          # atomic c_mode
        (256, 32, (16, 4, 4, cout, G.K4S2_TP), G.OUT_F32, {}),                 # M / 4 % 128
        (512, 128, (32, 4, 4, cout, G.K4S2_TP), G.OUT_F32, {}),                # K != 4 cin
        (480, 32, (32, 3, 5, cout, G.K4S2_TP), G.OUT_F32, {}),                 # odd h / w
        (512, 32, (32, 4, 4, cout, G.K4S2_TP), G.OUT_F32, {"b_mode": G.OPB_ROWK}),
        (512, 72, (8, 8, 8, cout, G.DOWN2), G.OUT_F32, {"b_mode": G.OPB_ROWK}),  # DOWN2 stays refused
    ]
    for M, K, conv, c_mode, over in cases:
        kw = {**tp, **over}
        cv = G.Conv(*conv, cout)
        assert G.gemm_refused(M, N, K, kw["a_mode"], kw["b_mode"], c_mode, cv), (M, K, conv)
        refused(O, M, N, K, dy, wf, tile=4, c_mode=c_mode, conv=conv, **kw)
    a, b = put(ints(g, 64, 40), False), put(ints(g, 64, 40), False)
    for M, N, K, am, bm in ((64, 20, 36, G.OPA_ROWK, G.OPB_ROWK), (20, 16, 64, G.OPA_ROWM, G.OPB_ROWN),
                            (64, 20, 40, G.OPA_ROWK, G.OPB_ROWN)):
        assert G.gemm_refused(M, N, K, am, bm, G.OUT_F32)
        refused(O, M, N, K, a, b, tile=4, a_mode=am, b_mode=bm)


@pytest.mark.parametrize("rs", [G.NONE, G.UP2])
@pytest.mark.parametrize("h,w,batch,fast", [(4, 4, 5, True), (8, 8, 3, True), (16, 16, 1, True), (6, 6, 5, False),
                                             (12, 4, 3, False)])
def test_im2col_wgrad_operand(O, rs, h, w, batch, fast):
    """OPB_IM2COL, the weight gradient's B operand (k = output pixel): the b_pix fast path
    (w | 64 and hw | 64 or 64 | hw) and the general path, 3x3 and nearest-up, cin 8 and 24, into
    the channels-last accumulate and the reference-layout scatter.  Catches a k-tile's image / row
    base taken from the wrong pixel, the x bound checked against h, padding rows of the next image."""
    K, M = batch * h * w, 40
    for strided in (False, True):
        for cin in (8, 24):
            g = _gen(1400 + 10 * rs + h * w + cin + int(strided))
            dy = put(ints(g, K, M), strided)
            x = put(ints(g, src_pixels(batch, h, w, rs), cin), strided)
            kw = dict(tile=4, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL, conv=(batch, h, w, cin, rs),
                      bias_grad=ints(g, M), expect={"b_pix": fast},
                      what=f"wgrad operand rs={rs} {h}x{w} cin={cin} strided={int(strided)}")
            run(O, M, 9 * cin, K, dy, x, c_mode=G.OUT_F32_ACCUM, c_init=ints(g, M, 9 * cin), strided_out=strided, **kw)
            if cin == 8:
                run(O, M, 9 * cin, K, dy, x, c_mode=G.OUT_F32_ATOMIC_CONVW, convw_cin=cin, c_init=ints(g, M, 9 * cin),
                    **kw)


# ====================================================================== 5. halo tiles
HALO_TWIN = {16: 4, 17: 2, 18: 1, 22: 3}  # halo tile -> the ring tile of the same BM x BN
HALO_CASES = [(3, 4, 8, 0), (64, 2, 8, 0), (64, 2, 192, 0), (16, 4, 24, 0), (16, 4, 64, 2), (16, 4, 128, 0), (2, 16, 8, 0),
              (2, 16, 24, 2), (2, 16, 64, 0), (2, 16, 128, 0), (1, 32, 8, 0), (1, 32, 24, 0), (16, 4, 24, 3),
              (2, 16, 8, 3), (16, 4, 8, 4), (2, 16, 24, 4), (64, 2, 64, 4)]  # batch, h = w, cin, resample


@functools.lru_cache(maxsize=None)
def _halo_inputs(batch, h, cin, rs, strided):
    """Operands and the fp64 reference of one halo case, shared by the eight tiles."""
    g = _gen(1500 + 7 * batch + h + cin + 100 * rs + int(strided))
    T = G.taps(rs)[0]
    M, N = batch * h * h, 40
    x = put(ints(g, src_pixels(batch, h, h, rs), cin), strided)
    wf = put(ints(g, N, T * cin), strided)
    bias = putv(ints(g, N))
    P = problem(M, N, T * cin, x, wf, G.OPA_IM2COL, G.OPB_ROWK, G.OUT_F32, (batch, h, h, cin, rs), bias=bias)
    assert G.exact_bound(P) < LIMIT
    out = dict(x=x, wf=wf, bias=bias, ref=G.result(P))
    if rs == G.NONE:  # the input gradient of the same conv: dY [M][cin'] with cin' = cin, weights [cin][9 * N]
        dy = put(ints(g, M, cin), strided)
        wd = put(ints(g, cin, 9 * N), strided)
        Pd = problem(M, N, 9 * cin, dy, wd, G.OPA_IM2COL, G.OPB_CONV_DGRAD, G.OUT_F32, (batch, h, h, cin, rs),
                     conv_cout=cin)
        assert G.exact_bound(Pd) < LIMIT
        out.update(dy=dy, wd=wd, dref=G.result(Pd))
    return out


@pytest.mark.parametrize("tile", sorted(G.HALO_TILES))
def test_halo_tiles(O, tile):
    """Halo tiles: the tile's whole conv-input window staged once in LDS -- whole images (2x2,
    4x4: ni > 1) and rows of one image (16x16, 32x32), every forward resample and the 3x3 input
    gradient, the channel counts at which the bank swizzle (xmsk / xsh) changes.  Exact, and
    bitwise the ring tile of the same shape.  What halo_fits declines the library must refuse.
    Catches: a window row / column off by one at an image edge, the window of the NEXT image read
    for ni > 1, the swizzle applied on one side only, a tap's window offset at stride 2."""
    ran = refusals = 0
    for batch, h, cin, rs in HALO_CASES:
        for strided in (False, True):
            c = _halo_inputs(batch, h, cin, rs, strided)
            M, N, T = batch * h * h, 40, G.taps(rs)[0]
            fits = O.halo_fits(tile, batch, h, h, cin, rs)
            assert fits == G.halo_ok(tile, batch, h, h, cin, rs)
            kw = dict(a_mode=G.OPA_IM2COL, c_mode=G.OUT_F32, conv=(batch, h, h, cin, rs))
            what = f"halo tile {tile} B={batch} h={h} cin={cin} rs={rs} strided={int(strided)}"
            if not fits:
                refused(O, M, N, T * cin, c["x"], c["wf"], tile=tile, **kw)
                refusals += 1
                continue
            ni, rows = G.halo_window(tile, h, h)   # whole images (ni of them) or rows of one image
            bm = G.HALO_TILES[tile][0]
            assert (ni, rows) == ((bm // (h * h), h) if h <= 4 else (1, min(h, bm // h))), what
            assert (ni > 1) == (h <= 4)
            out = run(O, M, N, T * cin, c["x"], c["wf"], tile=tile, bias=c["bias"], ref=c["ref"], strided_out=strided,
                      expect={"nkt": [G.ktiles(T * cin, 64)], "a_tapk": cin % 64 == 0, "ws_path": False}, what=what,
                      **kw)[0]
            ran += 1
            if tile in HALO_TWIN:
                twin = run(O, M, N, T * cin, c["x"], c["wf"], tile=HALO_TWIN[tile], bias=c["bias"], ref=c["ref"],
                           strided_out=strided, what=what + " twin", **kw)[0]
                assert R.same_bits(out.view, twin.view)
            if rs != G.NONE:
                continue
            kd = dict(a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD, c_mode=G.OUT_F32, conv=(batch, h, h, cin, rs),
                      conv_cout=cin)
            run(O, M, N, 9 * cin, c["dy"], c["wd"], tile=tile, ref=c["dref"], strided_out=strided, what=what + " dgrad",
                **kd)
    assert ran and refusals


@pytest.mark.parametrize("tile", [16, 17, 22])
@pytest.mark.parametrize("split", [2, 4])
def test_halo_split_k(O, tile, split):
    """Halo tiles with split-K over source-channel slices (each split stages its slice of the
    window and runs every tap over it): through the finalize (F32, bf16 + bias + resid) and the
    in-kernel combine; the refusals halo_fits predicts (cin % (64 split), window too large)."""
    N = 40
    for batch, h, cin, rs in ((16, 4, 128, 0), (64, 2, 256, 0), (4, 8, 256, 0), (16, 4, 256, 2), (16, 4, 192, 0),
                              (16, 4, 128, 4)):
        strided = (batch + cin) % 3 == 0
        g = _gen(1600 + batch + cin + split)
        T = G.taps(rs)[0]
        M, K = batch * h * h, T * cin
        x = put(ints(g, src_pixels(batch, h, h, rs), cin), strided)
        wf = put(ints(g, N, K), strided)
        kw = dict(a_mode=G.OPA_IM2COL, conv=(batch, h, h, cin, rs))
        fits = O.halo_fits(tile, batch, h, h, cin, rs, split)
        assert fits == G.halo_ok(tile, batch, h, h, cin, rs, split)
        if not fits:
            refused(O, M, N, K, x, wf, tile=tile, split=split, **kw)
            continue
        what = f"halo split tile {tile} split {split} B={batch} h={h} cin={cin} rs={rs}"
        exp = {"nkt": [T * (cin // split // 64)] * split, "ws_path": True}
        run(O, M, N, K, x, wf, tile=tile, split=split, c_mode=G.OUT_F32, strided_out=strided,
            expect={**exp, "folded": False}, what=what + " f32", **kw)
        bias, resid = putv(ints(g, N)), put(ints(g, M, N), strided)
        for fold in (False, True):
            run(O, M, N, K, x, wf, tile=tile, split=split, fold=fold, alpha=0.5, bias=bias, resid=resid,
                strided_out=strided, expect={**exp, "folded": fold}, what=what + f" bf16 fold={fold}", **kw)
        if rs == G.NONE:
            dy, wd = put(ints(g, M, cin), strided), put(ints(g, cin, 9 * N), strided)
            run(O, M, N, 9 * cin, dy, wd, tile=tile, split=split, a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD,
                c_mode=G.OUT_F32, conv=(batch, h, h, cin, rs), conv_cout=cin, strided_out=strided, expect=exp,
                what=what + " dgrad")


# ====================================================================== 6. WG3 / WGL
def _wg3_batch(h, tile, split):
    """The smallest batch whose chunk of whole images gives every wave a stage."""
    ni, rows = (1 if h == 16 else 2), (4 if h == 4 else 2)
    b = ni
    while ((b // ni) * (h // rows)) % G.wg3_waves(tile):
        b += ni
    return b * split


@pytest.mark.parametrize("rs", [G.NONE, G.UP2])
@pytest.mark.parametrize("h", [4, 8, 16])
@pytest.mark.parametrize("tile", [32, 33, 34])
def test_wg3(O, tile, h, rs):
    """The 3x3 weight-gradient kernel: its per-wave halo staging, the 9 tap offsets, the
    cross-wave sum and the slab path (split 2), onto a non-zero dW, with and without bias_grad.
    Catches: a halo border row not zeroed (the neighbouring image's row read instead), two taps
    swapped, a wave's partial dropped from the sum, a chunk starting at the wrong image."""
    for split in (1, 2):
        batch = _wg3_batch(h, tile, split)
        K = batch * h * h
        for (cout, cin), strided in (((32, 16), False), ((64, 48), True)):
            g = _gen(1700 + tile + h + 10 * rs + split + cout)
            assert G.wg3_ok(tile, batch, h, h, cout, cin, rs, cout + 24 * strided, cin + 24 * strided,
                            G.OUT_F32_ACCUM, split)
            dy = put(ints(g, K, cout), strided)
            x = put(ints(g, src_pixels(batch, h, h, rs), cin), strided)
            for with_bg in (True, False):
                run(O, cout, 9 * cin, K, dy, x, tile=tile, split=split, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL,
                    c_mode=G.OUT_F32_ACCUM, conv=(batch, h, h, cin, rs), c_init=ints(g, cout, 9 * cin),
                    bias_grad=ints(g, cout) if with_bg else None, strided_out=strided,
                    expect={"ws_path": split > 1, "folded": False},
                    what=f"wg3 tile {tile} h={h} rs={rs} split={split} {cout}x{cin} bias_grad={with_bg}")
    # refusals, as wg3_split / the copy of wg3_check predict
    g = _gen(1799)
    batch = _wg3_batch(h, tile, 1)
    dy, x = put(ints(g, batch * h * h, 32), False), put(ints(g, batch * h * h, 24), False)
    for cout, cin, sp in ((32, 24, 1), (24, 16, 1), (32, 16, 3)):
        assert not G.wg3_ok(tile, batch, h, h, cout, cin, G.NONE, 32, 24, G.OUT_F32_ACCUM, sp)
        if sp == 1:
            assert O.wg3_split(batch, h, h, cout, cin, G.NONE, 32, 24, G.OUT_F32_ACCUM, tile=tile) is None
        refused(O, cout, 9 * cin, batch * h * h, dy, x, tile=tile, split=sp, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL,
                c_mode=G.OUT_F32_ACCUM, conv=(batch, h, h, cin, G.NONE))


@pytest.mark.parametrize("M,N", [(64, 64), (128, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("kmul", [1, 2, 3])
def test_wgl(O, M, N, kmul):
    """The linear weight-gradient kernel (64 x 64 parts, waves split the tokens) with every split
    its check admits, plain and through slabs, onto a non-zero dW, with bias_grad."""
    K = 256 * kmul
    for split in (1, 2, 3, 4, 6):
        ok = K % (split * 128) == 0
        for strided in (False, True):
            g = _gen(1800 + M + N // 64 + kmul + split + int(strided))
            dy, x = put(ints(g, K, M), strided), put(ints(g, K, N), strided)
            assert ok == G.wgl_ok(M, N, K, dy.stride(0), x.stride(0), G.OUT_F32_ACCUM, split)
            kw = dict(tile=36, split=split, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN)
            if not ok:
                refused(O, M, N, K, dy, x, c_mode=G.OUT_F32_ACCUM, **kw)
                continue
            run(O, M, N, K, dy, x, c_mode=G.OUT_F32_ACCUM, c_init=ints(g, M, N), bias_grad=ints(g, M),
                strided_out=strided, expect={"ws_path": split > 1}, what=f"wgl {M}x{N} K={K} split={split}", **kw)
            if split == 1:
                run(O, M, N, K, dy, x, c_mode=G.OUT_F32, strided_out=strided, what=f"wgl {M}x{N} K={K} f32", **kw)
    g = _gen(1899)
    dy, x = put(ints(g, 256, 72), False), put(ints(g, 256, 64), False)
    assert O.wgl_split(72, 64, 256, 72, 64, G.OUT_F32_ACCUM) is None and not G.wgl_ok(72, 64, 256, 72, 64, 4, 1)
    refused(O, 72, 64, 256, dy, x, tile=36, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32_ACCUM)


# ====================================================================== 7. paired and grouped launches
def _pair_problem(O, kind, g, strided):
    """(wgrad kwargs, dgrad kwargs) of one layer's backward for run() / gemm_args."""
    if kind == "conv":   # 3x3 conv, 8x8 images: WG3 (tile 32) + input gradient on tile 4
        batch, h, cin, cout = 4, 8, 16, 32
        pix = batch * h * h
        dy, x, wf = put(ints(g, pix, cout), strided), put(ints(g, pix, cin), strided), put(ints(g, cout, 9 * cin), strided)
        w = dict(M=cout, N=9 * cin, K=pix, a=dy, b=x, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL, c_mode=G.OUT_F32_ACCUM,
                 conv=(batch, h, h, cin, G.NONE))
        d = dict(M=pix, N=cin, K=9 * cout, a=dy, b=wf, a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD, c_mode=G.OUT_BF16,
                 conv=(batch, h, h, cout, G.NONE), conv_cout=cout)
        return w, d
    T, cout, cin = 520, 64, 128   # linear: dW [cout][cin] = dY^T x, dx = dY W
    if kind == "wgl":
        T = 512
    dy, x, wt = put(ints(g, T, cout), strided), put(ints(g, T, cin), strided), put(ints(g, cout, cin), strided)
    w = dict(M=cout, N=cin, K=T, a=dy, b=x, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32_ACCUM)
    d = dict(M=T, N=cin, K=cout, a=dy, b=wt, a_mode=G.OPA_ROWK, b_mode=G.OPB_ROWN, c_mode=G.OUT_BF16)
    return w, d


PAIR_PLANS = {  # plan -> (wgrad tile, wgrad split, dgrad tile, dgrad split, the grid gemm_restate.pair_route names)
    "gemm2": (4, 3, 4, 1, "gemm2"), "gemm2_ring4": (5, 2, 4, 1, "gemm2"), "gemm2_k128": (7, 2, 7, 1, "gemm2"),
    "gemm2_ring8": (10, 2, 9, 1, "gemm2"), "gemm2_fin2": (4, 3, 4, 2, "gemm2"), "wgl": (36, 2, 4, 1, "wgl_pair"),
    "conv": (32, 2, 4, 1, "wg3_pair"), "conv_gemm2": (4, 2, 4, 2, "gemm2"), "conv_halo": (32, 1, 16, 1, "wg3_pair")}


def _args_of(O, p, out, bg, tile, split, off):
    L = O.L
    cg = None
    if p.get("conv") is not None:
        c = p["conv"]
        src = p["a"] if p["a_mode"] == G.OPA_IM2COL else p["b"]
        cg = L.ConvGeom(batch=c[0], h=c[1], w=c[2], cin=c[3], resample=c[4], ld_src=src.stride(0))
    a = O.gemm_args(p["M"], p["N"], p["K"], p["a"], p["a"].stride(0), p["b"], p["b"].stride(0), out.view,
                    out.view.stride(0), a_mode=p["a_mode"], b_mode=p["b_mode"], c_mode=p["c_mode"], conv=cg,
                    conv_cout=p.get("conv_cout", 0), split_k=split, tile=tile, ws_offset=off,
                    bias_grad=None if bg is None else bg.view)
    assert (a.tile, a.split_k) == (tile, split)
    return a


@pytest.mark.parametrize("plan", sorted(PAIR_PLANS))
def test_pairs(O, plan):
    """encdiff_gemm_pair_*: a layer's weight and input gradient in one grid (gemm2_kernel, the WG3
    and WGL paired forms, a halo input gradient), twice in a row so that the first weight
    gradient's finalize rides in the second launch; then once through encdiff_gemm_pair itself
    (nothing deferred: where both problems leave slabs, ONE finalize launch serves both,
    gemm_finalize2_kernel).  Both halves are exact and bitwise the two separate launches; the copy
    of the pairing rules (gemm_restate.pair_route) pins the fused grid each plan names.  Catches a block range of the 1-D grid given to the wrong problem, the
    riding finalize reading the other workspace half, the second problem's tile using the first's
    LDS layout."""
    wt, ws, dt_, ds, route = PAIR_PLANS[plan]
    kind = "conv" if plan.startswith("conv") else ("wgl" if plan == "wgl" else "lin")
    both = G.ws_path(G.OUT_F32_ACCUM, ws) and G.ws_path(G.OUT_BF16, ds)
    assert both == (plan in ("gemm2_fin2", "conv_gemm2"))
    for strided in (False, True):
        g = _gen(1900 + len(plan) + int(strided))
        w, d = _pair_problem(O, kind, g, strided)
        dw0, db0 = ints(g, w["M"], w["N"]), ints(g, w["M"])
        # separately: exact against the restatement
        so = run(O, w["M"], w["N"], w["K"], w["a"], w["b"], tile=wt, split=ws, c_init=dw0, bias_grad=db0,
                 strided_out=strided, what=f"pair {plan} wgrad alone",
                 **{k: v for k, v in w.items() if k not in ("M", "N", "K", "a", "b")})
        sd = run(O, d["M"], d["N"], d["K"], d["a"], d["b"], tile=dt_, split=ds, strided_out=strided,
                 what=f"pair {plan} dgrad alone", **{k: v for k, v in d.items() if k not in ("M", "N", "K", "a", "b")})
        # paired, two layers in a row
        outs = []
        for i in range(2):
            dw = Guard(w["M"], w["N"], F32, strided=strided, init=dw0.to(E.dev))
            db = Guard(1, w["M"], F32, init=db0.reshape(1, -1).to(E.dev))
            dx = Guard(d["M"], d["N"], BF16, strided=strided,
                       init=torch.full((d["M"], d["N"]), NAN, dtype=BF16, device=E.dev))
            if i == 0:
                O.flush()
                O._workspace().fill_(NAN)
            O.gemm_pair(lambda off: _args_of(O, w, dw, db, wt, ws, off), lambda off: _args_of(O, d, dx, None, dt_, ds, off))
            outs.append((dw, db, dx))
        O.flush()
        # encdiff_gemm_pair: no deferral, both finalizes behind the grid
        dw = Guard(w["M"], w["N"], F32, strided=strided, init=dw0.to(E.dev))
        db = Guard(1, w["M"], F32, init=db0.reshape(1, -1).to(E.dev))
        dx = Guard(d["M"], d["N"], BF16, strided=strided,
                   init=torch.full((d["M"], d["N"]), NAN, dtype=BF16, device=E.dev))
        aw = _args_of(O, w, dw, db, wt, ws, 0)
        ad = _args_of(O, d, dx, None, dt_, ds, O.ws_floats(aw))
        assert not ad.split_counters, "the input gradient's slabs are meant for the finalize"
        got = G.pair_route((w["a_mode"], w["b_mode"]), aw.tile, (d["a_mode"], d["b_mode"]), ad.tile)
        assert got == route, f"pair {plan}: pairing changed: {got}, this case needs {route}"
        if route == "gemm2":
            assert G.pair_finalize(O.ws_floats(aw) > 0, O.ws_floats(ad) > 0) == ("both" if both else "w")
        O._workspace()[:O.ws_floats(aw) + O.ws_floats(ad)].fill_(NAN)
        O.check(O.lib.encdiff_gemm_pair(ctypes.byref(aw), ctypes.byref(ad), O._s()), "encdiff_gemm_pair")
        outs.append((dw, db, dx))
        torch.cuda.synchronize()
        assert tickets_zero(O)
        for dw, db, dx in outs:
            for gd in (dw, db, dx):
                gd.check()
            assert R.same_bits(dw.view, so[0].view), \
                f"pair {plan}: dW: " + first_bad(dw.view.contiguous(), so[0].view.contiguous())
            assert R.same_bits(db.view, so[1].view), f"pair {plan}: db"
            assert R.same_bits(dx.view, sd[0].view), \
                f"pair {plan}: dx: " + first_bad(dx.view.contiguous(), sd[0].view.contiguous())


def test_pair_dx_deferred(O):
    """encdiff_gemm_pair_dx with the INPUT gradient's finalize deferred: after the paired launch dx
    is untouched, encdiff_gemm_finalize completes it; the weight gradient's own deferred finalize
    runs at flush()."""
    for strided in (False, True):
        g = _gen(1990 + int(strided))
        w, d = _pair_problem(O, "lin", g, strided)
        d = {**d, "K": 5 * 64 - 8}
        d["a"], d["b"] = put(ints(g, d["M"], d["K"]), strided), put(ints(g, d["K"], d["N"]), strided)
        dw0 = ints(g, w["M"], w["N"])
        dw = Guard(w["M"], w["N"], F32, strided=strided, init=dw0.to(E.dev))
        dx = Guard(d["M"], d["N"], BF16, strided=strided, init=torch.full((d["M"], d["N"]), NAN, dtype=BF16, device=E.dev))
        Pw = problem(w["M"], w["N"], w["K"], w["a"], w["b"], w["a_mode"], w["b_mode"], w["c_mode"], c_in=dw.view.clone())
        Pd = problem(d["M"], d["N"], d["K"], d["a"], d["b"], d["a_mode"], d["b_mode"], d["c_mode"])
        assert max(G.exact_bound(Pw), G.exact_bound(Pd)) < LIMIT
        O.flush()
        O._workspace().fill_(NAN)
        left = O.gemm_pair(lambda off: _args_of(O, w, dw, None, 4, 3, off), lambda off: _args_of(O, d, dx, None, 4, 4, off),
                           defer_dx=True)
        torch.cuda.synchronize()
        assert left is not None and left.split_k == 4 and not left.split_counters
        assert R.same_bits(dx.buf, dx.before), "dx written although its finalize was deferred"
        O.finalize(left)
        O.flush()
        torch.cuda.synchronize()
        dw.check()
        dx.check()
        assert same(dw.view, G.result(Pw)["c"].to(F32)) and same(dx.view, G.result(Pd)["c"].to(F32).to(BF16))


def test_wgrad_group_exact(O):
    """encdiff_wgrad_group_plan / _launch on three problems -- a linear layer (WGL body), a 3x3
    conv (WG3 body), a narrow linear on the generic tile and one deep enough to be cut into chunks
    combined in the kernel -- exact, onto non-zero dW / bias gradients; the tickets are left zero
    and a relaunch of the planned group gives the same bits."""
    g = _gen(2000)
    probs, checks = [], []
    lin = [(512, 64, 128), (8192, 64, 64), (200, 72, 40)]   # tokens, cout, cin (the second: two chunks)
    for i, (T, cout, cin) in enumerate(lin):
        dy, x = put(ints(g, T, cout), i % 2 == 1), put(ints(g, T, cin), i % 2 == 1)
        p = dict(M=cout, N=cin, K=T, a=dy, b=x, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32_ACCUM)
        probs.append((p, ints(g, cout, cin), ints(g, cout)))
    for batch, h, cin, cout, rs in ((4, 8, 16, 32, G.NONE), (32, 16, 16, 32, G.UP2)):  # the second: chunked
        pix = batch * h * h
        dy, x = put(ints(g, pix, cout), True), put(ints(g, src_pixels(batch, h, h, rs), cin), True)
        p = dict(M=cout, N=9 * cin, K=pix, a=dy, b=x, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL, c_mode=G.OUT_F32_ACCUM,
                 conv=(batch, h, h, cin, rs))
        probs.append((p, ints(g, cout, 9 * cin), ints(g, cout)))
    grp = O.WgradGroup()
    for p, dw0, db0 in probs:
        dw = Guard(p["M"], p["N"], F32, init=dw0.to(E.dev))
        db = Guard(1, p["M"], F32, init=db0.reshape(1, -1).to(E.dev))
        P = problem(p["M"], p["N"], p["K"], p["a"], p["b"], p["a_mode"], p["b_mode"], p["c_mode"], p.get("conv"),
                    c_in=dw.view.clone(), bias_grad_in=db.view[0].clone())
        assert G.exact_bound(P) < LIMIT
        grp.add(_args_of(O, p, dw, db, 4, 1, 0))
        checks.append((dw, db, G.result(P)))
    O.flush()
    O._workspace().fill_(NAN)
    assert tickets_zero(O)
    grp.launch()
    torch.cuda.synchronize()
    assert tickets_zero(O)
    for i, (dw, db, ref) in enumerate(checks):
        dw.check()
        db.check()
        assert same(dw.view, ref["c"].to(F32)), \
            f"group problem {i}: dW: " + first_bad(dw.view.contiguous(), ref["c"].to(F32))
        assert same(db.view[0], ref["bias_grad"].to(F32)), f"group problem {i}: bias gradient"
    first = [(dw.view.clone(), db.view.clone()) for dw, db, _ in checks]
    for (dw, db, _), (p, dw0, db0) in zip(checks, probs):
        dw.view.copy_(dw0)
        db.view.copy_(db0.reshape(1, -1))
    host, devb = list(grp._plans.values())[0][:2]
    O.check(O.lib.encdiff_wgrad_group_launch(ctypes.addressof(host), devb.data_ptr(), O._s()), "group relaunch")
    torch.cuda.synchronize()
    assert tickets_zero(O)
    for (dw, db, _), (f_dw, f_db) in zip(checks, first):
        assert R.same_bits(dw.view, f_dw) and R.same_bits(db.view, f_db)


# ====================================================================== 8. fp32 GEMM (fp32.hip)
F32_PAIRS = ["rowk_rowk", "im2col_rowk", "rowk_rown", "im2col_dgrad", "rowm_rown", "rowm_im2col"]


def _f32_case(O, pair, g, strided, exact, accumulate):
    """One ops.gemm_f32 launch; returns (out Guard, bias-gradient Guard or None, Problem)."""
    L = O.L
    draw = (lambda *s: ints(g, *s)) if exact else (lambda *s: gauss(g, *s))
    batch, h, w, rs = 3, 6, 4, (G.UP2 if strided else G.NONE)
    pix = batch * h * w
    cv = bias = resid = bgi = None
    cc = 0
    if pair == "rowk_rowk":
        M, N, K = 77, 50, 92
        a, b, am, bm = put(draw(M, K), strided, F32), put(draw(N, K), strided, F32), G.OPA_ROWK, G.OPB_ROWK
        bias, resid = putv(draw(N)), put(draw(M, N), strided, F32)
    elif pair == "rowk_rown":
        M, N, K = 77, 50, 91
        a, b, am, bm = put(draw(M, K), strided, F32), put(draw(K, N), strided, F32), G.OPA_ROWK, G.OPB_ROWN
    elif pair == "rowm_rown":
        M, N, K = 77, 50, 91
        a, b, am, bm = put(draw(K, M), strided, F32), put(draw(K, N), strided, F32), G.OPA_ROWM, G.OPB_ROWN
        bgi = draw(M)
    elif pair == "im2col_rowk":
        cin, N = 12, 50
        M, K, cv = pix, 9 * cin, (batch, h, w, cin, rs)
        a, b, am, bm = put(draw(src_pixels(batch, h, w, rs), cin), strided, F32), put(draw(N, K), strided, F32), 1, 0
        bias = putv(draw(N))
    elif pair == "im2col_dgrad":
        cc, N = 11, 50
        M, K, cv = pix, 9 * cc, (batch, h, w, cc, G.NONE)
        a, b, am, bm = put(draw(pix, cc), strided, F32), put(draw(cc, 9 * N), strided, F32), 1, 2
    else:
        cin, M = 5, 77
        N, K, cv = 9 * cin, pix, (batch, h, w, cin, rs)
        a, b, am, bm = put(draw(pix, M), strided, F32), put(draw(src_pixels(batch, h, w, rs), cin), strided, F32), 2, 3
        bgi = draw(M)
    c0 = draw(M, N) if accumulate else torch.full((M, N), NAN)
    out = Guard(M, N, F32, strided=strided, init=c0.to(E.dev))
    bg = None if bgi is None else Guard(1, M, F32, init=bgi.reshape(1, -1).to(E.dev))
    alpha = 1.0 if not exact else (0.5 if accumulate else -2.0)
    P = problem(M, N, K, a, b, am, bm, G.OUT_F32_ACCUM if accumulate else G.OUT_F32, cv, conv_cout=cc, alpha=alpha,
                bias=bias, resid=resid, c_in=out.view.clone() if accumulate else None,
                bias_grad_in=None if bg is None else bg.view[0].clone())
    cg = None
    if cv is not None:
        cg = L.ConvGeom(batch=batch, h=h, w=w, cin=cv[3], resample=cv[4], ld_src=P.conv.ld_src)
    O.gemm_f32(M, N, K, a, a.stride(0), b, b.stride(0), out.view, out.view.stride(0), a_mode=am, b_mode=bm, conv=cg,
               bias=bias, resid=resid, accumulate=accumulate, alpha=alpha, conv_cout=cc,
               bias_grad=None if bg is None else bg.view)
    torch.cuda.synchronize()
    out.check()
    if bg is not None:
        bg.check()
    return out, bg, P


@pytest.mark.parametrize("pair", F32_PAIRS)
def test_gemm_f32(O, pair):
    """The fp32 GEMM on the same restatement: exact integer cases for its six mode pairs, stored
    and accumulating, ragged M, N, K (K % 4 != 0 where the pair allows it), contiguous and strided
    (the strided convs use UP2); then one Gaussian case per pair under the fp32 rule."""
    for strided in (False, True):
        for accumulate in (False, True):
            g = _gen(2100 + int(strided) + 2 * int(accumulate))
            out, bg, P = _f32_case(O, pair, g, strided, True, accumulate)
            assert G.exact_bound(P) < LIMIT
            ref = G.result(P)
            assert same(out.view, ref["c"].to(F32)), f"fp32 {pair}: " + first_bad(out.view.contiguous(), ref["c"].to(F32))
            if bg is not None:
                assert same(bg.view[0], ref["bias_grad"].to(F32))
    out, bg, P = _f32_case(O, pair, _gen(2150), True, False, True)
    ref, t32 = G.result(P, F64), G.result(P, F32)
    assert_f32_rule(out.view, ref["c"], t32["c"], f"fp32 gemm {pair}")
    if bg is not None:
        assert_f32_rule(bg.view[0], ref["bias_grad"], t32["bias_grad"], f"fp32 gemm {pair} bias_grad")


# ====================================================================== 9. rounded cases
ROUNDED = ["rowk_rowk", "im2col_rowk", "rowk_rown", "im2col_dgrad", "rowm_rown", "rowm_im2col", "halo", "wg3", "wgl",
           "split_finalize", "split_fold"]


@pytest.mark.parametrize("name", ROUNDED)
def test_rounded(O, name):
    """Gaussian bf16 operands (non-integer magnitudes): fp32 outputs under the fp32 rule, bf16
    outputs under the bf16 rule, floor = 4 x the largest |restatement in fp32 - fp64|.  A bf16
    accumulator, a partial sum rounded to bf16 between k-tiles or slabs, would miss these by
    orders of magnitude."""
    g = _gen(2200 + ROUNDED.index(name))
    s = True
    kw = dict(exact=False, strided_out=s, what=f"rounded {name}")
    if name in ("rowk_rowk", "split_finalize", "split_fold"):
        M, N, K = 88, 72, 456
        a, b = put(gauss(g, M, K), s), put(gauss(g, N, K, scale=K ** -0.5), s)
        split = 1 if name == "rowk_rowk" else 3
        kw["expect"] = {"nkt": G.split_ktiles(K, 64, split), "ws_path": split > 1, "folded": name == "split_fold"}
        rb = run(O, M, N, K, a, b, tile=4, split=split, fold=name == "split_fold", bias=putv(gauss(g, N)),
                 resid=put(gauss(g, M, N), s), **kw)
        rf = run(O, M, N, K, a, b, tile=4, split=split, fold=name == "split_fold", c_mode=G.OUT_F32, **kw)
    elif name == "rowk_rown":
        M, N, K = 88, 72, 456
        a, b = put(gauss(g, M, K), s), put(gauss(g, K, N, scale=K ** -0.5), s)
        kw["expect"] = {"nkt": [8], "vec": True, "xcd": False}
        rb = run(O, M, N, K, a, b, tile=4, b_mode=G.OPB_ROWN, **kw)
        rf = run(O, M, N, K, a, b, tile=4, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32, **kw)
    elif name in ("im2col_rowk", "halo"):
        batch, h, cin, N = (5, 4, 24, 40) if name == "im2col_rowk" else (16, 4, 24, 40)
        tile = 4 if name == "im2col_rowk" else 16
        M, K = batch * h * h, 9 * cin
        a, b = put(gauss(g, M, cin), s), put(gauss(g, N, K, scale=K ** -0.5), s)
        c = dict(a_mode=G.OPA_IM2COL, conv=(batch, h, h, cin, G.NONE))
        kw["expect"] = {"nkt": [4], "a_tapk": False, "ws_path": False}
        rb = run(O, M, N, K, a, b, tile=tile, bias=putv(gauss(g, N)), **c, **kw)
        rf = run(O, M, N, K, a, b, tile=tile, c_mode=G.OUT_F32, **c, **kw)
    elif name == "im2col_dgrad":
        batch, h, cout, N = 5, 4, 24, 40
        M, K = batch * h * h, 9 * cout
        a, b = put(gauss(g, M, cout), s), put(gauss(g, cout, 9 * N, scale=K ** -0.5), s)
        c = dict(a_mode=G.OPA_IM2COL, b_mode=G.OPB_CONV_DGRAD, conv=(batch, h, h, cout, G.NONE), conv_cout=cout)
        kw["expect"] = {"nkt": [4], "a_tapk": False, "b_tapk": False}
        rb = run(O, M, N, K, a, b, tile=4, **c, **kw)
        rf = run(O, M, N, K, a, b, tile=4, c_mode=G.OUT_F32, **c, **kw)
    elif name in ("rowm_rown", "wgl"):
        M, N, K = (88, 72, 456) if name == "rowm_rown" else (64, 128, 512)
        tile, split = (4, 1) if name == "rowm_rown" else (36, 2)
        a, b = put(gauss(g, K, M), s), put(gauss(g, K, N), s)
        rb = None
        kw["expect"] = {"ws_path": split > 1, "folded": False, "xcd": True}
        assert name != "wgl" or G.wgl_ok(M, N, K, a.stride(0), b.stride(0), G.OUT_F32_ACCUM, split)
        rf = run(O, M, N, K, a, b, tile=tile, split=split, a_mode=G.OPA_ROWM, b_mode=G.OPB_ROWN, c_mode=G.OUT_F32_ACCUM,
                 c_init=gauss(g, M, N), bias_grad=gauss(g, M), **kw)
    else:  # rowm_im2col, wg3
        batch, h, cin, cout = (5, 6, 8, 40) if name == "rowm_im2col" else (4, 8, 16, 32)
        tile, split = (4, 1) if name == "rowm_im2col" else (32, 2)
        K = batch * h * h
        a, b = put(gauss(g, K, cout), s), put(gauss(g, K, cin), s)
        rb = None
        kw["expect"] = {"ws_path": split > 1, "folded": False, "xcd": True}
        assert name != "wg3" or G.wg3_ok(tile, batch, h, h, cout, cin, G.NONE, a.stride(0), b.stride(0), G.OUT_F32_ACCUM, split)
        rf = run(O, cout, 9 * cin, K, a, b, tile=tile, split=split, a_mode=G.OPA_ROWM, b_mode=G.OPB_IM2COL,
                 c_mode=G.OUT_F32_ACCUM, conv=(batch, h, h, cin, G.NONE), c_init=gauss(g, cout, 9 * cin),
                 bias_grad=gauss(g, cout), **kw)
    if rb is not None:
        out, _, ref, P = rb
        assert_bf16_rule(out.view, ref["c"], G.result(P, F32)["c"], f"rounded {name} bf16")
    out, bg, ref, P = rf
    t32 = G.result(P, F32)
    assert_f32_rule(out.view, ref["c"], t32["c"], f"rounded {name} f32")
    if bg is not None:
        assert_f32_rule(bg.view[0], ref["bias_grad"], t32["bias_grad"], f"rounded {name} bias_grad")
