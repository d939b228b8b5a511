"""Per-element tests of the normalisation kernels on the MI355X: csrc/norm.hip (GroupNorm + FiLM +
SiLU and LayerNorm, bf16, forward and backward) and the four norm kernels of csrc/fp32.hip.

Rules (tests/elementwise_restate.py), reference = tests/norm_restate.py evaluated in fp64 on the
case's own (already rounded) inputs, floor = 4 x the largest |the same restatement in fp32 - fp64|:
  * bf16 outputs (y, dsilu, dx):        |out - ref64| <= 2^-7 |ref64| + floor
  * fp32 outputs (stats, partials, dfilm): |out - ref64| <= floor + 2^-22 |ref64|
  * every output is a view in a sentinel-filled buffer whose other bytes must not change; fp32
    outputs are pre-filled with NaN, so an unwritten (image, slice, channel) shows.
The backward is fed statistics (and silu'(z) rows) rounded from the fp64 reference, not the
kernel's own; one chained case per family uses the kernel's forward outputs.
Every GroupNorm case asserts the path it means to reach through the copy of the dispatch in
norm_restate.GnPath -- if the slice heuristic changes, the case fails instead of testing nothing.

No output needed a wider floor.  The one derived addition: dx + a RESAMPLED resid is rounded to
bf16 before the adjoint is added, so next to a rounding boundary of dx two correct evaluations
differ by a bf16 ulp of dx; norm_restate.two_rounding_slack() adds exactly that, per element, and
only where the floor-wide interval around the fp64 dx straddles a boundary (1 - 7 % of the elements).
Largest floors measured on the MI355X (the whole file takes 4.8 s):
  GroupNorm bf16: y 1.9e-4, dsilu 3.8e-5, dx 8.4e-6, mean 1.3e-6, rstd 7.8e-4 (HW = 1, three
    elements per group: rstd up to 300), d gamma 1.4e-4, d beta 1.2e-4, d scale 1.2e-4, d shift 5.6e-5;
    conditioning at |mean| / std = 64: rstd 2.7e-2 (rstd = 33; the kernel's own error 5.6e-3), y 4.5e-3
  LayerNorm bf16: y 5.0e-6, dx 3.9e-6, mean 1.5e-7, rstd 8.1e-7, d gamma 4.2e-5, d beta 4.8e-6
  fp32 kernels: y 4.7e-3 and mean 2.4e-3 at mean = 4096 std (1.9e-5 / 5.5e-7 at ratio 1), dx 2.6e-5,
    rstd 6.5e-6, d gamma 1.3e-5, d beta 1.2e-5, d scale 7.8e-6, d shift 5.5e-6

Kernel branch -> test
  gn_fwd_kernel, slice_partials butterfly 3 levels (nvc 1..8, nval 1) ..... test_gn_fwd_pow2[nvc1..nvc8]
  slice_partials butterfly 2 / 1 / 0 levels (nvc 16 / 32 / 64: nval 2 / 4 / 8,
    owner_mask == 0, rows = 256 / nvc at 64), HW = 1 ....................... test_gn_fwd_pow2[nvc16..nvc64]
  slice_partials LDS rows (nvc 3 .. 48; 16 idle threads at 24 / 40 / 48) .. test_gn_fwd_npow2
  gn_xcd_index: grid % 8 == 0 (remapped) and odd grids (identity) ........ test_gn_fwd_pow2 (B = 64), test_gn_fwd_other[odd-grid*]
  cpg = 1, groups = 8, non-square, largest tiled slice, untiled slice ..... test_gn_fwd_other
  FiLM (ld_film = 2C + 32) / SiLU / dsilu / eps / strided x, y, dsilu ...... every forward test (four option sets)
  y bitwise equal with and without dsilu .................................. _fwd_case (every dsilu case)
  gn_fwd_kernel with x from deferred split-K slabs (x_from, gn_stream_in's
    slab branch): bitwise against finalize-then-forward ................... test_gpu_ops.py::test_groupnorm_from_deferred_finalize
  gn_fwd_stats_kernel: nseg = 1 + PF guards, nvc 3, B = 64 ................ test_gn_fwd_in_stats[stats-*]
  gn_group_stats_kernel + gn_apply_kernel: C = 32 / 512 / 128, partial
    last row block, HW % 256 != 0 ........................................ test_gn_fwd_in_stats[group-*]
  in_stats given but unusable -> gn_fwd_kernel ............................ test_gn_fwd_in_stats[self-*]
  refusals: cs > 512, C % 8, C % groups, misaligned dsilu ................. test_gn_refusals
  one-pass variance under |mean| / std = 1, 16, 64 ........................ test_gn_fwd_conditioning
  gn_bwd_kernel<false> / <false,false,true>, `one`, pow2 and non-pow2 ..... test_gn_bwd[one-*]
  gn_bwd_kernel not `one`, untiled pass 2 (partial last batch) ............ test_gn_bwd[untiled-96x32x32]
  gn_bwd_kernel not `one`, LDS-tiled pass 2 (non-slab) .................... test_gn_bwd[tiled-192x13x13]
  gn_bwd_kernel with 8 groups; a grid that is no multiple of 8 (no remap) . test_gn_bwd[one-groups8], [one-odd-grid]
  accumulate / resid / both, FiLM + ld_dfilm = 2C + 32, ld_part > C ....... test_gn_bwd (option sets)
  gn_bwd_kernel<false,true> / <false,true,true>: DOWN2 / UP2 of dy, resid . test_gn_bwd_resample
  refusals: DOWN2 with odd h / w, resid_resample without resid ............ test_gn_bwd_refusals
  gn_bwd_kernel<true> / <true,false,true> (dy_from slabs), tiled and
    untiled pass 2, split 2 / 8 / 16 (gn_slab_row's z-groups) ............. test_gn_bwd_dy_from
  forward -> backward on the kernel's own stats / dsilu ................... test_gn_chained
  ln_fwd_kernel<64..512>: rows 1, RPB - 1, k RPB + 5, strided ............. test_ln_fwd
  ln_fwd_kernel grid cap 4096 + grid-stride loop (C = 512, 64) ............ test_ln_fwd_grid_cap
  ln_bwd_kernel<64..512>: empty blocks write zeros, U = 2 pair with a
    missing second row, two full rounds + tail; plain / accumulate / resid  test_ln_bwd
  ln_bwd_kernel dy_from slabs ............................................. test_ln_bwd_dy_from
  forward -> backward on the kernel's own stats ........................... test_ln_chained
  gn_f32_kernel / gn_bwd_f32_kernel (HW = 1, cpg 3, FiLM, SiLU, accumulate,
    resid; |mean| / std = 1, 64, 4096) .................................... test_gn_f32
  ln_f32_kernel / ln_bwd_f32_kernel (rows tail, empty parts) .............. test_ln_f32
(The weight-gradient fold riding in gn_bwd_kernel has its own bitwise test in test_gpu_unet.py.)
"""
import ctypes

import pytest
import torch

import elementwise_restate as R
import norm_restate as N
from test_gpu_elementwise import Guard, place, rnd, _gen, assert_bf16_rule, assert_f32_rule

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    import encdiff_amd._lib as lib
    assert (lib.RESAMPLE_DOWN2, lib.RESAMPLE_UP2) == (N.DOWN2, N.UP2)
    return ops


def nan_guard(rows, cols, strided=False):
    return Guard(rows, cols, F32, strided=strided, init=torch.full((rows, cols), NAN, device=dev))


def film_of(g, B, C):
    """[B][2C + 32] fp32; the 32 columns behind scale | shift are NaN (they must not be read)."""
    E = rnd(g, B, 2 * C + 32, scale=0.3)
    E[:, 2 * C:] = NAN
    return E


def affine_of(g, C):
    return 1 + rnd(g, C, scale=0.3), rnd(g, C, scale=0.3)


def expect_path(p, **want):
    assert p.ok
    for k, v in want.items():
        assert getattr(p, k) == v, f"dispatch changed: {k} = {getattr(p, k)}, this case needs {v}"


# option sets of the forward cases: (film, silu, dsilu, eps, strided)
FWD_OPTS = [(True, True, True, 1e-5, False), (False, True, False, 1e-6, True),
            (True, False, False, 1e-6, True), (False, True, True, 1e-5, True)]


# ====================================================================== 1. GroupNorm forward
def _fwd_case(O, C, h, w, B, opts, seed, groups=32, in_stats=False, x=None, what=""):
    """One forward launch checked per element; returns (x, gamma, beta, E, y, ds, stats) views."""
    film, silu, dsilu, eps, strided = opts
    g = _gen(seed)
    HW = h * w
    x = rnd(g, B * HW, C, scale=2.0, dtype=F32).add_(0.5).to(BF16) if x is None else x
    x = place(x, strided)
    gamma, beta = affine_of(g, C)
    E = film_of(g, B, C) if film else None
    y = Guard(B * HW, C, BF16, strided=strided)
    ds = Guard(B * HW, C, BF16, strided=strided) if dsilu else None
    st = nan_guard(B * groups, 2)
    seg = None
    if in_stats:
        seg = N.segment_stats(x, B, HW, ld=C + 8) if HW % 64 == 0 else torch.full((2 * B, C + 8), NAN, device=dev)
    geom = O.Geom(B, h, w)
    kw = dict(film=E, ld_film=2 * C + 32 if film else 0, groups=groups, in_stats=seg)
    O.groupnorm_fwd(x, geom, gamma, beta, y.view, st.view, eps, silu, dsilu=ds.view if ds else None, **kw)
    torch.cuda.synchronize()
    for o in (y, ds, st):
        if o is not None:
            o.check()
    what = f"{what} C{C} {h}x{w} B{B} film{int(film)} silu{int(silu)} ds{int(dsilu)} eps{eps} strided{int(strided)}"
    if in_stats and HW % 64 == 0:
        stat = lambda dt: N.gn_stats_from_segments(seg, B, HW, C, groups, eps, dt)
    else:
        stat = lambda dt: N.gn_stats_onepass(x, B, HW, groups, eps, dt)
    (m64, r64), (m32, r32) = stat(F64), stat(F32)
    got = st.view.reshape(B, groups, 2)
    assert_f32_rule(got[..., 0], m64, m32, what + " mean")
    assert_f32_rule(got[..., 1], r64, r32, what + " rstd")
    y64, d64 = N.gn_apply(x, B, HW, gamma, beta, m64, r64, film=E, use_silu=silu, dtype=F64)
    y32, d32 = N.gn_apply(x, B, HW, gamma, beta, m32, r32, film=E, use_silu=silu, dtype=F32)
    assert_bf16_rule(y.view, y64, y32, what + " y")
    if dsilu:
        assert_bf16_rule(ds.view, d64, d32, what + " dsilu")
        y2 = Guard(B * HW, C, BF16, strided=strided)
        st2 = nan_guard(B * groups, 2)
        O.groupnorm_fwd(x, geom, gamma, beta, y2.view, st2.view, eps, silu, **kw)
        torch.cuda.synchronize()
        y2.check()
        assert R.same_bits(y2.view, y.view), what + ": y differs with / without dsilu"
        assert R.same_bits(st2.view, st.view), what + ": stats differ with / without dsilu"
    return x, gamma, beta, E, y, ds, st


def _fwd_all_opts(O, C, h, w, B, seed, **kw):
    for i, opts in enumerate(FWD_OPTS):
        _fwd_case(O, C, h, w, B, opts, seed + i, **kw)


POW2 = [(64, 16, 16, 2, 1), (128, 8, 8, 2, 2), (64, 4, 4, 2, 4), (64, 2, 2, 2, 8), (128, 1, 1, 2, 16),
        (128, 4, 4, 64, 16), (256, 2, 2, 64, 32), (512, 1, 1, 64, 64)]


@pytest.mark.parametrize("C,h,w,B,nvc", POW2, ids=[f"nvc{c[4]}-B{c[3]}" for c in POW2])
def test_gn_fwd_pow2(O, C, h, w, B, nvc):
    """Self-reducing forward, power-of-two slice widths.  nvc >= 16 runs the butterfly with fewer
    than three levels (each owner lane writes nval = 2 / 4 / 8 channel totals, every lane an owner);
    nvc = 64 has no shuffle at all and 256 / 64 LDS rows.  Catches: nval or the channel offset `c`
    wrong for a short butterfly (a group's statistics from half its channels), owner lanes missing
    (NaN statistics from unwritten LDS), rows mis-counted at nvc = 64, the XCD remap of a grid that
    is a multiple of 8 sending two workgroups to one (image, slice) (NaN statistics elsewhere)."""
    p = N.GnPath(C, h * w, B)
    expect_path(p, nvc=nvc, pow2=True, fwd="self", fwd_tiled=True, nval={1: 1, 2: 1, 4: 1, 8: 1, 16: 2, 32: 4, 64: 8}[nvc])
    if B == 64:
        assert p.grid % 8 == 0
    _fwd_all_opts(O, C, h, w, B, 100 + nvc + B)


NPOW2 = [(96, 8, 8, 2, 3), (320, 4, 4, 2, 5), (96, 4, 4, 2, 6), (320, 2, 2, 2, 10), (96, 1, 1, 2, 12),
         (320, 4, 4, 64, 20), (192, 1, 1, 2, 24), (320, 1, 1, 2, 40), (384, 1, 1, 2, 48)]


@pytest.mark.parametrize("C,h,w,B,nvc", NPOW2, ids=[f"nvc{c[4]}-B{c[3]}" for c in NPOW2])
def test_gn_fwd_npow2(O, C, h, w, B, nvc):
    """Self-reducing forward, slice widths that are no power of two: every pixel lane's partial row
    goes through LDS.  At nvc = 24 / 40 / 48 the last 16 threads have no pixel lane.  Catches: idle
    threads writing an LDS row or a y row (guard), np rows mis-counted, tv / tp swapped."""
    p = N.GnPath(C, h * w, B)
    expect_path(p, nvc=nvc, pow2=False, fwd="self", fwd_tiled=True)
    if nvc in (24, 40, 48):
        assert p.idle == 16
    _fwd_all_opts(O, C, h, w, B, 200 + nvc + B)


OTHER = {  # name: (C, h, w, B, groups, expectations)
    "cpg1": (32, 8, 8, 2, 32, dict(nvc=2, cpg=1)),
    "groups8": (64, 4, 4, 2, 8, dict(nvc=4, cpg=8)),
    "nonsquare-3x5": (64, 3, 5, 2, 32, dict(nvc=4)),
    "odd-grid6": (64, 4, 4, 3, 32, dict(nvc=4, grid=6)),
    "odd-grid3": (96, 1, 1, 3, 32, dict(nvc=12, grid=3)),
    "largest-tile-64x64": (64, 64, 64, 2, 32, dict(nvc=1, fwd_tiled=True)),
    "untiled-96x64x64": (96, 64, 64, 2, 32, dict(nvc=3, fwd_tiled=False)),
}


@pytest.mark.parametrize("name", list(OTHER))
def test_gn_fwd_other(O, name):
    """One channel per group, 8 groups, a non-square image, grids that are no multiple of 8 (no
    remap), the largest slice that still fits the LDS tile (4096 vectors, 16 rows per thread) and a
    slice that does not (12288 vectors: pass 2 re-reads x from memory).  Catches: group index from
    the wrong cpg, h taken for w, the remap applied to a grid it is not a bijection on, a tile index
    past the tile, the untiled re-read using the tile's row stride."""
    C, h, w, B, groups, want = OTHER[name]
    expect_path(N.GnPath(C, h * w, B, groups), fwd="self", **want)
    opts = FWD_OPTS[:2] if h * w >= 4096 else FWD_OPTS
    for i, o in enumerate(opts):
        _fwd_case(O, C, h, w, B, o, 300 + i + C, groups=groups, what=name)


IN_STATS = {  # name: (C, h, w, B, forward kernel, expectations)
    "stats-nseg1-pf-guards": (64, 8, 8, 2, "stats", dict(nvc=2, np=128)),   # HW = 64 < 4 np: one preload row valid
    "stats-nvc3": (192, 16, 16, 2, "stats", dict(nvc=3)),
    "stats-B64": (64, 16, 16, 64, "stats", dict(nvc=4)),
    "stats-nvc3-32x32": (192, 32, 32, 2, "stats", dict(nvc=3)),             # 24 vectors of C do not divide 256
    "group-C32": (32, 32, 32, 2, "group_apply", {}),
    "group-C512": (512, 32, 32, 1, "group_apply", {}),
    "group-C128-32x48": (128, 32, 48, 2, "group_apply", {}),                # 1536 = 6 x 256
    "group-C128-33x64": (128, 33, 64, 2, "group_apply", {}),                # 2112 % 256 = 64: partial last block
    "self-hw-not-64": (64, 3, 5, 2, "self", dict(nvc=4)),
    "self-segments-too-many": (320, 64, 64, 1, "self", dict(nvc=5, fwd_tiled=False)),
}


@pytest.mark.parametrize("name", list(IN_STATS))
def test_gn_fwd_in_stats(O, name):
    """Forward from the producer's per-64-row segment sums (synthesised from x in fp64, rounded to
    fp32, ld = C + 8 with NaN padding).  The reference statistics are formed from those sums.
    Catches: the PF = 4 preload reading rows >= HW, segment / moment index swapped ((2 (b nseg +
    sg) + k) ld + c), inv_n without cpg, the apply kernel's last row block running past HW or
    stopping short, np = 4 at C = 512, a fallback that reads the unusable in_stats anyway."""
    C, h, w, B, kern, want = IN_STATS[name]
    expect_path(N.GnPath(C, h * w, B, in_stats=True, ld_in_stats=C + 8), fwd=kern, **want)
    opts = [FWD_OPTS[0], FWD_OPTS[2]] if h * w >= 1024 else FWD_OPTS
    for i, o in enumerate(opts):
        _fwd_case(O, C, h, w, B, o, 400 + i + C, in_stats=True, what=name)


def test_gn_refusals(O):
    """Shapes the kernels cannot run are refused with an error and nothing is written."""
    from encdiff_amd._lib import HipError
    g = _gen(5)

    def run(C, B, groups=32, ds_off=None):
        x = rnd(g, B, C, dtype=BF16)
        gamma, beta = affine_of(g, C)
        y = Guard(B, C, BF16)
        st = nan_guard(B * groups, 2)
        ds = None
        if ds_off is not None:
            ds = torch.zeros(B * C + 16, dtype=BF16, device=dev)[ds_off:ds_off + B * C].view(B, C)
        with pytest.raises(HipError):
            O.groupnorm_fwd(x, O.Geom(B, 1, 1), gamma, beta, y.view, st.view, 1e-5, True, groups=groups, dsilu=ds)
        torch.cuda.synchronize()
        assert R.same_bits(y.buf, y.before) and R.same_bits(st.buf, st.before)

    assert not N.GnPath(640, 1, 64).ok and N.GnPath(640, 1, 64).cs == 640
    run(640, 64)            # slice of 640 channels > 512
    run(36, 2, groups=4)    # C % 8 != 0
    run(72, 2, groups=32)   # C % groups != 0
    run(64, 2, ds_off=4)    # dsilu 8 bytes off a 16-byte boundary


def _offset_x(g, C, HW, B, ratio):
    """x with per-group offsets so that |mean| / std ~ ratio.  bf16 keeps 8 significant bits, so
    the offset sits just below a power of two (1.9375 .. 2: ulp 2^-7) and sigma = offset / ratio is
    15.5 ulp at ratio 16 (4 bits below sigma) and 3.9 ulp at ratio 64 (2 bits: all that bf16 can
    hold there, mean / ulp <= 256).  The references are formed from the rounded inputs."""
    if ratio == 1:
        off, sigma = 1.0, 1.0
    else:
        off, sigma = 1.9375, 1.9375 / ratio
    sign = torch.where(torch.arange(32) % 2 == 0, 1.0, -1.0).repeat_interleave(C // 32)
    v = torch.randn(B * HW, C, generator=g) * sigma + off * sign
    return v.to(BF16).to(dev)


@pytest.mark.parametrize("ratio", [1, 16, 64])
@pytest.mark.parametrize("C,h,w,nvc", [(64, 16, 16, 1), (96, 8, 8, 3)])
def test_gn_fwd_conditioning(O, C, h, w, nvc, ratio):
    """var = E[x^2] - mean^2 in one fp32 pass loses log2(ratio^2) bits: groups with |mean| / std = 1,
    16, 64 (alternating sign per group).  The fp32 evaluation of the same one-pass form sets the
    floor, so this pins that the kernel's summation is no worse than a plain fp32 one-pass sum; it
    would catch sums kept in bf16, a mean subtracted after rounding, or a variance clamped wrongly."""
    expect_path(N.GnPath(C, h * w, 2), nvc=nvc, fwd="self")
    x = _offset_x(_gen(ratio + C), C, h * w, 2, ratio)
    for i, opts in enumerate(FWD_OPTS[:2]):
        _fwd_case(O, C, h, w, 2, opts, 500 + i, x=x, what=f"ratio{ratio}")


# ====================================================================== 2. GroupNorm backward
# option sets: (film, silu, use_dsilu, accumulate, resid, strided (also ld_part > C))
BWD_OPTS = [(True, True, False, False, False, False), (True, True, True, True, False, True),
            (False, True, True, False, True, True), (False, True, False, True, True, False),
            (True, False, False, False, True, True)]


def _bwd_inputs(g, C, HW, B, groups, film, silu, eps=1e-5):
    x = rnd(g, B * HW, C, scale=2.0, dtype=F32).add_(0.5).to(BF16)
    gamma, beta = affine_of(g, C)
    E = film_of(g, B, C) if film else None
    m64, r64 = N.gn_stats_twopass(x, B, HW, groups, eps)
    mean, rstd = m64.float(), r64.float()   # the statistics the backward is given
    dsr = None
    if silu:
        dsr = N.gn_apply(x, B, HW, gamma, beta, mean, rstd, film=E, use_silu=True)[1].to(BF16)
    return x, gamma, beta, E, mean, rstd, dsr


def _bwd_check(O, what, x, geom, gamma, beta, E, mean, rstd, dsr, dy_eff, opts, groups, call_kw, ref_kw, seed):
    """Launch the backward on guarded outputs and compare with the restatement (dy_eff: the dy the
    kernel's arithmetic sees; call_kw: how it is handed over)."""
    film, silu, use_ds, accumulate, resid, strided = opts
    B, HW, C = geom.batch, geom.h * geom.w, x.shape[1]
    g = _gen(seed)
    prev = rnd(g, B * HW, C, dtype=BF16) if accumulate else None
    dx = Guard(B * HW, C, BF16, strided=strided, init=prev)
    dgp, dbp = nan_guard(B, C, strided), nan_guard(B, C, strided)
    dE = nan_guard(B, 2 * C + 32) if film else None
    stats = torch.stack([mean, rstd], dim=-1).contiguous()
    O.groupnorm_bwd(place(x, strided), geom, gamma, beta, stats, 1e-5, silu, dx=dx.view, dgamma_part=dgp.view,
                    dbeta_part=dbp.view, film=E, ld_film=2 * C + 32 if film else 0, dfilm=dE.view if film else None,
                    ld_dfilm=2 * C + 32 if film else 0, accumulate=accumulate, groups=groups,
                    ld_part=dgp.view.stride(0), dsilu=place(dsr, strided) if (silu and use_ds) else None, **call_kw)
    torch.cuda.synchronize()
    for o in (dx, dgp, dbp, dE):
        if o is not None:
            o.check()
    kw = dict(film=E, use_silu=silu, dsilu=dsr if use_ds else None, prev=prev, **ref_kw)
    o64 = N.gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy_eff, dtype=F64, **kw)
    o32 = N.gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy_eff, dtype=F32, **kw)
    what = f"{what} film{int(film)} silu{int(silu)} ds{int(use_ds)} acc{int(accumulate)} resid{int(resid)} strided{int(strided)}"
    if "dx_pre" in o64:  # dx rounded to bf16, then + the resid adjoint: floor from the unrounded terms
        fpre = R.floor_of(o32["dx_pre"], o64["dx_pre"])
        floor = fpre + R.floor_of(o32["resid_adj"], o64["resid_adj"])
        slack = N.two_rounding_slack(o64["dx_pre"], fpre)
        err = (dx.view.double() - o64["dx"]).abs()
        ex = err - (2.0 ** -7 * o64["dx"].abs() + floor + slack)
        print(f"{what} dx: floor {floor:.3e} max|out-ref| {err.max().item():.3e} excess {ex.max().item():.3e} "
              f"(elements next to a rounding boundary of dx: {int((slack > 0).sum())})")
        assert ex.max().item() <= 0, f"{what} dx: element {int(ex.argmax())} exceeds the bound by {ex.max().item():.3e}"
    else:
        assert_bf16_rule(dx.view, o64["dx"], o32["dx"], what + " dx")
    assert_f32_rule(dgp.view, o64["dgamma"], o32["dgamma"], what + " dgamma_part")
    assert_f32_rule(dbp.view, o64["dbeta"], o32["dbeta"], what + " dbeta_part")
    if film:
        assert_f32_rule(dE.view[:, :C], o64["dscale"], o32["dscale"], what + " dfilm scale")
        assert_f32_rule(dE.view[:, C:2 * C], o64["dshift"], o32["dshift"], what + " dfilm shift")
        assert torch.isnan(dE.view[:, 2 * C:]).all(), what + ": dfilm columns behind 2C written"
    return dx, dgp, dbp, dE


def _bwd_case(O, C, h, w, B, opts, seed, groups=32, what=""):
    film, silu, use_ds, accumulate, resid, strided = opts
    g = _gen(seed)
    HW = h * w
    x, gamma, beta, E, mean, rstd, dsr = _bwd_inputs(g, C, HW, B, groups, film, silu)
    dy = rnd(g, B * HW, C, dtype=BF16)
    res = rnd(g, B * HW, C, dtype=BF16) if resid else None
    res_in = place(res, strided) if resid else None
    res_before = res_in.clone() if resid else None
    _bwd_check(O, f"{what} C{C} {h}x{w} B{B}", x, O.Geom(B, h, w), gamma, beta, E, mean, rstd, dsr, dy, opts, groups,
               dict(dy=place(dy, strided), resid=res_in), dict(resid=res), seed + 1)
    if resid:
        assert R.same_bits(res_in, res_before), "resid modified"


BWD = {  # name: (C, h, w, B, expectations)
    "one-nvc1": (64, 16, 16, 2, dict(nvc=1, one=True)),
    "one-nvc16-B64": (128, 4, 4, 64, dict(nvc=16, one=True, nval=2)),
    "one-nvc64-B64": (512, 1, 1, 64, dict(nvc=64, one=True, nval=8)),
    "one-nvc6": (96, 4, 4, 2, dict(nvc=6, one=True, pow2=False)),
    "one-nvc20-B64": (320, 4, 4, 64, dict(nvc=20, one=True, pow2=False)),
    "untiled-96x32x32": (96, 32, 32, 2, dict(nvc=3, np=85, one=False, bwd_tiled=False, last_batch_partial=True)),
    "tiled-192x13x13": (192, 13, 13, 64, dict(nvc=6, np=42, one=False, bwd_tiled=True)),
    "one-groups8": (64, 4, 4, 2, dict(nvc=4, cpg=8, one=True)),
    "one-odd-grid": (64, 4, 4, 3, dict(nvc=4, grid=6, one=True)),
}


@pytest.mark.parametrize("name", list(BWD))
def test_gn_bwd(O, name):
    """Backward from given statistics: dx, the per-image d gamma / d beta partials, d scale / d shift;
    SiLU recomputed and read from dsilu rows; accumulate, resid, both; ld_part > C; strided
    operands.  `one`: the thread's rows are one register-cached batch; otherwise pass 2 re-reads x /
    dy from memory (untiled; HW = 1024 is no multiple of 4 x 85 rows, so the last batch is partial)
    or from the LDS tiles (the only non-slab route into them).  Catches: the group terms m1 / m2
    from the wrong group or count, resid and the accumulated dx both dropped or added twice, a tile
    row index with the wrong stride, rows of a partial batch skipped or processed twice, d scale
    summed over dn instead of dz, partial rows written with stride C instead of ld_part."""
    C, h, w, B, want = BWD[name]
    groups = 8 if name == "one-groups8" else 32
    expect_path(N.GnPath(C, h * w, B, groups), **want)
    for i, opts in enumerate(BWD_OPTS):
        _bwd_case(O, C, h, w, B, opts, 600 + 10 * i + C, groups=groups, what=name)


RS_CASES = [(N.DOWN2, 0), (N.UP2, 0), (0, N.DOWN2), (0, N.UP2), (N.DOWN2, N.UP2), (N.UP2, N.DOWN2), (N.UP2, N.UP2)]


@pytest.mark.parametrize("C,h,w,one", [(64, 8, 8, True), (96, 32, 32, False)], ids=["one-64x8x8", "untiled-96x32x32"])
def test_gn_bwd_resample(O, C, h, w, one):
    """dy and / or resid given at the resolution behind a 2x resample (DOWN2: a quarter of the
    pixels, 0.25 x the parent; UP2: four times, the children summed ((a + b) + c) + d and rounded to
    bf16 as the separate adjoint kernel stores it).  The resid adjoint is added after dx's own
    rounding.  On the untiled slice pass 2 re-reads dy through the adjoint.  Catches: parent / child
    pixel index with the wrong width, the image offset of the resampled tensor taken from HW, pass 2
    reading dy rows at the plain resolution, the resid adjoint added before rounding or twice."""
    B = 2
    HW = h * w
    expect_path(N.GnPath(C, HW, B), one=one, bwd_tiled=False)
    hw_at = lambda mode: HW // 4 if mode == N.DOWN2 else HW * 4
    for i, (dy_rs, rs_rs) in enumerate(RS_CASES):
        opts = BWD_OPTS[i % 2][:3] + (i % 3 == 1, rs_rs != 0, i % 2 == 1)
        film, silu, use_ds, accumulate, resid, strided = opts
        g = _gen(700 + i + C)
        x, gamma, beta, E, mean, rstd, dsr = _bwd_inputs(g, C, HW, B, 32, film, silu)
        dy_at = rnd(g, B * (hw_at(dy_rs) if dy_rs else HW), C, dtype=BF16)
        dy_eff = N.resampled_dy(dy_at, dy_rs, B, h, w) if dy_rs else dy_at
        call = dict(dy=place(dy_at, strided), dy_resample=dy_rs, resid_resample=rs_rs)
        ref = {}
        if rs_rs:
            res_at = rnd(g, B * hw_at(rs_rs), C, dtype=BF16)
            call["resid"] = place(res_at, strided)
            ref["resid_adj"] = N.resample_adjoint(res_at, rs_rs, B, h, w, F64)
        _bwd_check(O, f"C{C} {h}x{w} dy_rs{dy_rs} resid_rs{rs_rs}", x, O.Geom(B, h, w), gamma, beta, E, mean, rstd,
                   dsr, dy_eff, opts, 32, call, ref, 750 + i)


def test_gn_bwd_refusals(O):
    """DOWN2 operands need even h and w; resid_resample needs a resid."""
    from encdiff_amd._lib import HipError
    g = _gen(8)
    C, B = 64, 2
    gamma, beta = affine_of(g, C)

    def run(h, w, **kw):
        HW = h * w
        x = rnd(g, B * HW, C, dtype=BF16)
        dy = rnd(g, B * max(1, HW // 4), C, dtype=BF16) if kw.get("dy_resample") else rnd(g, B * HW, C, dtype=BF16)
        dx = Guard(B * HW, C, BF16)
        dgp, dbp = nan_guard(B, C), nan_guard(B, C)
        stats = torch.ones(B, 32, 2, device=dev)
        with pytest.raises(HipError):
            O.groupnorm_bwd(x, O.Geom(B, h, w), gamma, beta, stats, 1e-5, False, dy, dx.view, dgp.view, dbp.view, **kw)
        torch.cuda.synchronize()
        assert R.same_bits(dx.buf, dx.before) and R.same_bits(dgp.buf, dgp.before)

    run(3, 4, dy_resample=N.DOWN2)
    run(4, 3, dy_resample=N.DOWN2)
    run(4, 4, resid_resample=N.UP2)
    run(3, 3, resid_resample=N.DOWN2, resid=rnd(g, B * 2, C, dtype=BF16))


def _producer(O, M, Nc, K, out, split, seed):
    """A linear GEMM [M][K] x [Nc][K]^T with `split` split-K slabs whose finalize can be deferred."""
    g = _gen(seed)
    a = rnd(g, M, K, dtype=BF16)
    wt = rnd(g, Nc, K, scale=K ** -0.5, dtype=BF16)
    bias = rnd(g, Nc, scale=0.1)
    args = O.gemm_args(M, Nc, K, a, K, wt, K, out, out.stride(0), bias=bias, split_k=split, tile=4)
    assert args.split_k == split and not args.split_counters
    return args, (a, wt, bias)


def _run_producer(O, args, defer):
    planned = ctypes.c_int(-1)
    O.check(O.lib.encdiff_gemm_ex(ctypes.byref(args), int(defer), ctypes.byref(planned), O._s()), "gemm_ex")
    assert planned.value == int(defer)


@pytest.mark.parametrize("use_ds", [False, True], ids=["recompute", "dsilu"])
@pytest.mark.parametrize("split", [2, 8, 16])
@pytest.mark.parametrize("C,h,w,tiled", [(64, 8, 8, True), (96, 32, 32, False)], ids=["tiled-64x8x8", "untiled-96x32x32"])
def test_gn_bwd_dy_from(O, C, h, w, tiled, split, use_ds):
    """dy combined from its producer's deferred split-K slabs inside the backward (split 2 and 8: one
    ordered sum; 16: four z-groups) against finalize-then-backward: dy, dx, both partials and dfilm
    bitwise equal, and dx within the per-element rule of the reference.  The slab instantiation never
    takes the `one` route; nvc HW <= 1024 runs its LDS-tiled pass 2, the larger slice re-reads the dy
    it wrote.  Catches: slabs added in another order than the finalize, dy not written back (or only
    for some rows), pass 2 reading a tile row that pass 1 did not fill."""
    B, HW = 2, h * w
    expect_path(N.GnPath(C, HW, B, slab=True), one=False, bwd_tiled=tiled)
    g = _gen(800 + split + C)
    film, silu = True, True
    x, gamma, beta, E, mean, rstd, dsr = _bwd_inputs(g, C, HW, B, 32, film, silu)
    stats = torch.stack([mean, rstd], dim=-1).contiguous()
    fold = O.SPLIT_FOLD
    O.SPLIT_FOLD = 0  # slabs for a finalize pass, not the in-kernel combine
    outs = []
    try:
        for defer in (False, True):
            dy = Guard(B * HW, C, BF16)
            args, keep = _producer(O, B * HW, C, 64 * split, dy.view, split, 850 + split)
            _run_producer(O, args, defer)
            dx = Guard(B * HW, C, BF16)
            dgp, dbp, dE = nan_guard(B, C), nan_guard(B, C), nan_guard(B, 2 * C + 32)
            O.groupnorm_bwd(x, O.Geom(B, h, w), gamma, beta, stats, 1e-5, silu, dy.view, dx.view, dgp.view, dbp.view,
                            film=E, ld_film=2 * C + 32, dfilm=dE.view, ld_dfilm=2 * C + 32,
                            dsilu=dsr if use_ds else None, dy_from=args if defer else None)
            torch.cuda.synchronize()
            for o in (dy, dx, dgp, dbp, dE):
                o.check()
            outs.append((dy, dx, dgp, dbp, dE))
    finally:
        O.SPLIT_FOLD = fold
    for u, v, nm in zip(outs[0], outs[1], ("dy", "dx", "dgamma_part", "dbeta_part", "dfilm")):
        assert R.same_bits(u.buf, v.buf), f"{nm} differs between finalize-then-backward and dy_from"
    dy, dx = outs[1][0].view, outs[1][1]
    kw = dict(film=E, use_silu=silu, dsilu=dsr if use_ds else None)
    o64 = N.gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy, dtype=F64, **kw)
    o32 = N.gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy, dtype=F32, **kw)
    assert_bf16_rule(dx.view, o64["dx"], o32["dx"], f"dy_from split{split} dx")
    assert_f32_rule(outs[1][2].view, o64["dgamma"], o32["dgamma"], f"dy_from split{split} dgamma_part")


@pytest.mark.parametrize("C,h,w,B", [(64, 16, 16, 2), (96, 32, 32, 2), (128, 4, 4, 64)],
                         ids=["one-nvc1", "untiled-nvc3", "one-nvc16"])
def test_gn_chained(O, C, h, w, B):
    """Forward (with dsilu) then backward on the kernel's OWN statistics and silu'(z) rows; the
    reference backward is fed those same outputs, so only the backward's arithmetic is judged while
    the hand-over format (stats pairs [B][G][2], dsilu rows) is the real one."""
    opts = (True, True, True, 1e-5, False)
    x, gamma, beta, E, y, ds, st = _fwd_case(O, C, h, w, B, opts, 900 + C, what="chained")
    g = _gen(901 + C)
    HW = h * w
    dy = rnd(g, B * HW, C, dtype=BF16)
    got = st.view.reshape(B, 32, 2)
    _bwd_check(O, f"chained C{C} {h}x{w} B{B}", x, O.Geom(B, h, w), gamma, beta, E, got[..., 0].contiguous(),
               got[..., 1].contiguous(), ds.view.contiguous(), dy, (True, True, True, False, False, False), 32,
               dict(dy=dy), {}, 902 + C)


# ====================================================================== 3. LayerNorm
LN_C = [64, 128, 256, 512]


def _ln_fwd_case(O, rows, C, strided, seed, eps=1e-5):
    g = _gen(seed)
    x = place(rnd(g, rows, C, dtype=F32).add_(0.3).to(BF16), strided)
    gamma, beta = affine_of(g, C)
    y = Guard(rows, C, BF16, strided=strided)
    st = nan_guard(rows, 2)
    O.layernorm_fwd(x, gamma, beta, y.view, st.view, eps)
    torch.cuda.synchronize()
    y.check()
    st.check()
    y64, m64, r64 = N.ln_fwd(x, gamma, beta, eps, F64)
    y32, m32, r32 = N.ln_fwd(x, gamma, beta, eps, F32)
    what = f"ln_fwd {rows}x{C} strided{int(strided)}"
    assert_f32_rule(st.view[:, 0], m64, m32, what + " mean")
    assert_f32_rule(st.view[:, 1], r64, r32, what + " rstd")
    assert_bf16_rule(y.view, y64, y32, what + " y")
    return x, gamma, beta, st


@pytest.mark.parametrize("C", LN_C)
def test_ln_fwd(O, C):
    """rows = 1, RPB - 1 (one partly filled block), 3 RPB + 5 (a tail block), contiguous and as
    column slices.  Catches: lanes of absent rows joining a present row's shuffle, the row stride
    taken for C, stats written by a lane other than the row's first, a dropped tail row."""
    rpb = N.ln_rpb(C)
    for rows in (1, rpb - 1, 3 * rpb + 5):
        for strided in (False, True):
            _ln_fwd_case(O, rows, C, strided, 1000 + rows + C)


@pytest.mark.parametrize("C", [512, 64])
def test_ln_fwd_grid_cap(O, C):
    """rows = 4096 RPB + RPB + 3: the grid is capped at 4096 blocks, so block 0 and 1 take a second
    trip through the grid-stride loop (the last one partial).  Catches: the loop stride without RPB,
    rows behind the cap never written (y sentinel, stats NaN)."""
    rpb = N.ln_rpb(C)
    rows = N.LN_FWD_GRID_CAP * rpb + rpb + 3
    _ln_fwd_case(O, rows, C, False, 1100 + C)


def _ln_bwd_case(O, rows, C, mode, strided, seed):
    g = _gen(seed)
    x = rnd(g, rows, C, dtype=F32).add_(0.3).to(BF16)
    gamma, _ = affine_of(g, C)
    _, m64, r64 = N.ln_fwd(x, gamma, gamma, 1e-5, F64)
    mean, rstd = m64.float(), r64.float()
    dy = rnd(g, rows, C, dtype=BF16)
    prev = rnd(g, rows, C, dtype=BF16) if mode == "accumulate" else None
    res = rnd(g, rows, C, dtype=BF16) if mode == "resid" else None
    res_in = place(res, strided) if res is not None else None
    res_before = res_in.clone() if res is not None else None
    dx = Guard(rows, C, BF16, strided=strided, init=prev)
    dgp, dbp = nan_guard(N.LN_PARTS, C, strided), nan_guard(N.LN_PARTS, C, strided)
    assert O.layernorm_parts(rows, C) == N.LN_PARTS
    O.layernorm_bwd(place(x, strided), gamma, torch.stack([mean, rstd], dim=-1).contiguous(), place(dy, strided),
                    dx.view, dgp.view, dbp.view, accumulate=mode == "accumulate", ld_part=dgp.view.stride(0),
                    resid=res_in)
    torch.cuda.synchronize()
    for o in (dx, dgp, dbp):
        o.check()
    if res is not None:
        assert R.same_bits(res_in, res_before), "resid modified"
    owner = N.ln_block_of_rows(rows, C)
    refs = []
    for dt in (F64, F32):
        d, tg, tb = N.ln_bwd(x, gamma, mean, rstd, dy, prev=prev, resid=res, dtype=dt)
        refs.append((d, N.partial_rows(tg, owner, N.LN_PARTS), N.partial_rows(tb, owner, N.LN_PARTS)))
    what = f"ln_bwd {rows}x{C} {mode} strided{int(strided)}"
    assert_bf16_rule(dx.view, refs[0][0], refs[1][0], what + " dx")
    assert_f32_rule(dgp.view, refs[0][1], refs[1][1], what + " dgamma_part")
    assert_f32_rule(dbp.view, refs[0][2], refs[1][2], what + " dbeta_part")
    used = torch.zeros(N.LN_PARTS, dtype=torch.bool)
    used[owner] = True
    empty = (~used).to(dev)
    assert (dgp.view[empty] == 0).all() and (dbp.view[empty] == 0).all(), what + ": empty blocks must write zeros"
    return int((~used).sum())


@pytest.mark.parametrize("mode", ["plain", "accumulate", "resid"])
@pytest.mark.parametrize("C", LN_C)
def test_ln_bwd(O, C, mode):
    """256 partial rows, block k owning rows {k RPB + rr + j 256 RPB}, two rows (j, j + 1) in flight.
    rows = 100 RPB + 3: blocks 101.. have no row and must write exact zeros over the NaN pre-fill;
    rows = 256 RPB + 40 RPB + 5: the second row of the pair exists for some blocks only;
    rows = 2 x 256 RPB + 7 RPB + 3: a second trip of the loop with a tail.
    Catches: the missing pair row read or written anyway, its partial added, empty blocks leaving
    their partial rows unwritten, resid added into itself (it must stay unchanged), accumulate
    reading dx after the store."""
    rpb = N.ln_rpb(C)
    n_empty = _ln_bwd_case(O, 100 * rpb + 3, C, mode, False, 1200 + C)
    assert n_empty == 256 - 101
    _ln_bwd_case(O, 256 * rpb + 40 * rpb + 5, C, mode, True, 1201 + C)
    _ln_bwd_case(O, 2 * 256 * rpb + 7 * rpb + 3, C, mode, mode == "plain", 1202 + C)


@pytest.mark.parametrize("split", [2, 16])
@pytest.mark.parametrize("C", [64, 256])
def test_ln_bwd_dy_from(O, C, split):
    """layernorm_bwd(dy_from=): dy, dx and both partials bitwise equal to finalize-then-backward."""
    rows = 256 * N.ln_rpb(C) + 37
    g = _gen(1300 + C)
    x = rnd(g, rows, C, dtype=F32).add_(0.3).to(BF16)
    gamma, _ = affine_of(g, C)
    _, m64, r64 = N.ln_fwd(x, gamma, gamma, 1e-5, F64)
    stats = torch.stack([m64.float(), r64.float()], dim=-1).contiguous()
    fold = O.SPLIT_FOLD
    O.SPLIT_FOLD = 0
    outs = []
    try:
        for defer in (False, True):
            dy = Guard(rows, C, BF16)
            args, keep = _producer(O, rows, C, 64 * split, dy.view, split, 1350 + split)
            _run_producer(O, args, defer)
            dx = Guard(rows, C, BF16)
            dgp, dbp = nan_guard(N.LN_PARTS, C), nan_guard(N.LN_PARTS, C)
            O.layernorm_bwd(x, gamma, stats, dy.view, dx.view, dgp.view, dbp.view, dy_from=args if defer else None)
            torch.cuda.synchronize()
            for o in (dy, dx, dgp, dbp):
                o.check()
            outs.append((dy, dx, dgp, dbp))
    finally:
        O.SPLIT_FOLD = fold
    for u, v, nm in zip(outs[0], outs[1], ("dy", "dx", "dgamma_part", "dbeta_part")):
        assert R.same_bits(u.buf, v.buf), f"{nm} differs between finalize-then-backward and dy_from"
    d64 = N.ln_bwd(x, gamma, stats[:, 0], stats[:, 1], outs[1][0].view, dtype=F64)[0]
    d32 = N.ln_bwd(x, gamma, stats[:, 0], stats[:, 1], outs[1][0].view, dtype=F32)[0]
    assert_bf16_rule(outs[1][1].view, d64, d32, f"ln dy_from C{C} split{split} dx")


@pytest.mark.parametrize("C", [64, 512])
def test_ln_chained(O, C):
    """Forward then backward on the kernel's own saved (mean, rstd) pairs."""
    rows = 5 * N.ln_rpb(C) + 3
    x, gamma, beta, st = _ln_fwd_case(O, rows, C, False, 1400 + C)
    g = _gen(1401 + C)
    dy = rnd(g, rows, C, dtype=BF16)
    dx = Guard(rows, C, BF16)
    dgp, dbp = nan_guard(N.LN_PARTS, C), nan_guard(N.LN_PARTS, C)
    O.layernorm_bwd(x, gamma, st.view, dy, dx.view, dgp.view, dbp.view)
    torch.cuda.synchronize()
    dx.check()
    mean, rstd = st.view[:, 0].contiguous(), st.view[:, 1].contiguous()
    owner = N.ln_block_of_rows(rows, C)
    d64, tg64, _ = N.ln_bwd(x, gamma, mean, rstd, dy, dtype=F64)
    d32, tg32, _ = N.ln_bwd(x, gamma, mean, rstd, dy, dtype=F32)
    assert_bf16_rule(dx.view, d64, d32, f"ln chained C{C} dx")
    assert_f32_rule(dgp.view, N.partial_rows(tg64, owner, N.LN_PARTS), N.partial_rows(tg32, owner, N.LN_PARTS),
                    f"ln chained C{C} dgamma_part")


# ====================================================================== 4. fp32 kernels (csrc/fp32.hip)
def _cond_x_f32(g, rows_shape, ratio, cpg=None):
    """fp32 x with mean = ratio x std; the sign alternates per group (cpg columns) or, cpg None, per row."""
    r, c = rows_shape
    if cpg is None:
        sign = torch.where(torch.arange(r) % 2 == 0, 1.0, -1.0)[:, None]
    else:
        sign = torch.where(torch.arange(c // cpg) % 2 == 0, 1.0, -1.0).repeat_interleave(cpg)
    return (torch.randn(r, c, generator=g) + ratio * sign).to(dev)


GN_F32 = [  # (C, h, w, B, groups, film, silu, accumulate, resid, ratio)
    (64, 1, 1, 2, 32, False, False, False, False, 1),       # HW = 1
    (96, 5, 3, 3, 32, True, True, False, False, 64),        # cpg 3 (256 threads: 85 per channel, one idle)
    (64, 16, 16, 2, 8, False, True, True, False, 4096),     # cpg 8, accumulate
    (160, 4, 4, 2, 32, True, False, False, True, 1),        # cpg 5, resid
]


@pytest.mark.parametrize("case", GN_F32, ids=[f"C{c[0]}-{c[1]}x{c[2]}-ratio{c[9]}" for c in GN_F32])
def test_gn_f32(O, case):
    """gn_f32_kernel and gn_bwd_f32_kernel, one workgroup per (image, group), two-pass statistics:
    they hold under |mean| / std up to 4096 where a one-pass variance would not.  Catches: a
    one-pass variance slipped in, the idle thread of a non-power-of-two cpg contributing, FiLM halves
    swapped, resid indexed with the output's row stride."""
    C, h, w, B, groups, film, silu, accumulate, resid, ratio = case
    g = _gen(1500 + C)
    HW = h * w
    x = _cond_x_f32(g, (B * HW, C), ratio, cpg=C // groups)
    gamma, beta = affine_of(g, C)
    E = film_of(g, B, C) if film else None
    y = Guard(B * HW, C, F32, strided=True)
    st = nan_guard(B * groups, 2)
    geom = O.Geom(B, h, w)
    O.groupnorm_f32(place(x, True), geom, gamma, beta, y.view, st.view, 1e-5, silu, film=E,
                    ld_film=2 * C + 32 if film else 0, groups=groups)
    torch.cuda.synchronize()
    y.check()
    st.check()
    what = f"gn_f32 C{C} {h}x{w} ratio{ratio}"
    (m64, r64), (m32, r32) = N.gn_stats_twopass(x, B, HW, groups, 1e-5, F64), N.gn_stats_twopass(x, B, HW, groups, 1e-5, F32)
    got = st.view.reshape(B, groups, 2)
    assert_f32_rule(got[..., 0], m64, m32, what + " mean")
    assert_f32_rule(got[..., 1], r64, r32, what + " rstd")
    y64 = N.gn_apply(x, B, HW, gamma, beta, m64, r64, film=E, use_silu=silu, dtype=F64, centred=True)[0]
    y32 = N.gn_apply(x, B, HW, gamma, beta, m32, r32, film=E, use_silu=silu, dtype=F32, centred=True)[0]
    assert_f32_rule(y.view, y64, y32, what + " y")
    # backward from the rounded reference statistics
    mean, rstd = m64.float(), r64.float()
    dy = rnd(g, B * HW, C)
    prev = rnd(g, B * HW, C) if accumulate else None
    res = rnd(g, B * HW, C) if resid else None
    dx = Guard(B * HW, C, F32, strided=True, init=prev)
    dgp, dbp = nan_guard(B, C, True), nan_guard(B, C, True)
    dE = nan_guard(B, 2 * C + 32) if film else None
    O.groupnorm_bwd_f32(place(x, True), geom, gamma, beta, torch.stack([mean, rstd], dim=-1).contiguous(), silu,
                        place(dy, True), dx.view, dgp.view, dbp.view, dgp.view.stride(0), film=E,
                        ld_film=2 * C + 32 if film else 0, dfilm=dE.view if film else None,
                        ld_dfilm=2 * C + 32 if film else 0, accumulate=accumulate,
                        resid=place(res, True) if resid else None, groups=groups)
    torch.cuda.synchronize()
    for o in (dx, dgp, dbp, dE):
        if o is not None:
            o.check()
    kw = dict(film=E, use_silu=silu, prev=prev, resid=res)
    o64 = N.gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy, dtype=F64, **kw)
    o32 = N.gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy, dtype=F32, **kw)
    assert_f32_rule(dx.view, o64["dx"], o32["dx"], what + " dx")
    assert_f32_rule(dgp.view, o64["dgamma"], o32["dgamma"], what + " dgamma_part")
    assert_f32_rule(dbp.view, o64["dbeta"], o32["dbeta"], what + " dbeta_part")
    if film:
        assert_f32_rule(dE.view[:, :C], o64["dscale"], o32["dscale"], what + " dfilm scale")
        assert_f32_rule(dE.view[:, C:2 * C], o64["dshift"], o32["dshift"], what + " dfilm shift")
        assert torch.isnan(dE.view[:, 2 * C:]).all()


LN_F32 = [(1, 64, 1, "plain", 16), (37, 320, 64, "accumulate", 16), (1027, 512, 4096, "resid", 256),
          (9, 72, 1, "plain", 16)]


@pytest.mark.parametrize("rows,C,ratio,mode,parts", LN_F32, ids=[f"{c[0]}x{c[1]}-ratio{c[2]}" for c in LN_F32])
def test_ln_f32(O, rows, C, ratio, mode, parts):
    """ln_f32_kernel (one wave per row, 4 rows per block: rows % 4 != 0 leaves waves without a row)
    and ln_bwd_f32_kernel (contiguous row ranges per part; parts behind the last row write zeros).
    C = 72 / 320 leave lanes without a channel in the last trip."""
    g = _gen(1600 + rows)
    x = _cond_x_f32(g, (rows, C), ratio)
    gamma, beta = affine_of(g, C)
    y = Guard(rows, C, F32, strided=True)
    st = nan_guard(rows, 2)
    O.layernorm_f32(place(x, True), gamma, beta, y.view, 1e-5, stats=st.view)
    torch.cuda.synchronize()
    y.check()
    st.check()
    what = f"ln_f32 {rows}x{C} ratio{ratio}"
    y64, m64, r64 = N.ln_fwd(x, gamma, beta, 1e-5, F64)
    y32, m32, r32 = N.ln_fwd(x, gamma, beta, 1e-5, F32)
    assert_f32_rule(st.view[:, 0], m64, m32, what + " mean")
    assert_f32_rule(st.view[:, 1], r64, r32, what + " rstd")
    assert_f32_rule(y.view, y64, y32, what + " y")
    mean, rstd = m64.float(), r64.float()
    dy = rnd(g, rows, C)
    prev = rnd(g, rows, C) if mode == "accumulate" else None
    res = rnd(g, rows, C) if mode == "resid" else None
    dx = Guard(rows, C, F32, strided=True, init=prev)
    dgp, dbp = nan_guard(parts, C, True), nan_guard(parts, C, True)
    O.layernorm_bwd_f32(place(x, True), gamma, torch.stack([mean, rstd], dim=-1).contiguous(), place(dy, True),
                        dx.view, dgp.view, dbp.view, parts, dgp.view.stride(0), accumulate=mode == "accumulate",
                        resid=place(res, True) if res is not None else None)
    torch.cuda.synchronize()
    for o in (dx, dgp, dbp):
        o.check()
    owner = N.ln_block_of_rows_f32(rows, parts)
    refs = []
    for dt in (F64, F32):
        d, tg, tb = N.ln_bwd(x, gamma, mean, rstd, dy, prev=prev, resid=res, dtype=dt)
        refs.append((d, N.partial_rows(tg, owner, parts), N.partial_rows(tb, owner, parts)))
    assert_f32_rule(dx.view, refs[0][0], refs[1][0], what + " dx")
    assert_f32_rule(dgp.view, refs[0][1], refs[1][1], what + " dgamma_part")
    assert_f32_rule(dbp.view, refs[0][2], refs[1][2], what + " dbeta_part")
