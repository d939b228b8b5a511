"""Pure-torch restatement of the GEMM's non-linear fused stagings and epilogues (csrc/gemm_tile.h):
AGN (EncdiffGemmArgs.agn_*: GroupNorm32 (+FiLM)(+SiLU) of the im2col source in the A staging), LNA
(lna_*: LayerNorm of the A rows in the staging), ln_y (LayerNorm of the produced rows in the
epilogue), OUT_BF16_GEGLU and OUT_BF16_GEGLU_BWD.  Written from include/encdiff_hip.h and the
modules the features replace -- ldm/modules/attention.py (GEGLU: x, gate = proj(x).chunk(2); x *
gelu(gate); nn.LayerNorm) and openaimodel_enc.py (ResBlock in_layers / out_layers: GroupNorm32,
out_norm(h) * (1 + scale) + shift, SiLU, conv 3x3) -- not from the kernels' loops.  The linear parts
are gemm_restate.Problem / result, the norms norm_restate.gn_stats_twopass / gn_apply / ln_fwd.

One function per stage, evaluated in a `dtype`: fp64 is the reference, fp32 the evaluation whose
distance from fp64 sets the additive floor.  tests/test_gpu_gemm_fused.py compares the kernels with
the stages; tests/test_gemm_fused_restate.py checks the stages against torch on the CPU, and proves
on the GPU cases' own inputs (the case tables below) that the bounds are sharp: a model of the
kernel stays inside them, a list of plausible index mistakes does not.

Bounds (the house rules of st_restate.py, nothing new): a stored bf16 value may differ by half a
bf16 ulp of the reference; an operand the kernel rounds without storing it (the normalised A chunk
of AGN / LNA, the d of GEGLU_BWD) stays unrounded in the reference and its half-ulp is carried
through the consumer with absolute values; the floor is measured.  The derived slacks are next to
their use: agn_stat_slack, lna_stat_slack.
"""
from dataclasses import replace
from types import SimpleNamespace as NS

import torch

import elementwise_restate as R
import gemm_restate as G
import norm_restate as N
import resconv_restate as RC
import st_restate as S

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
OUT_BF16_GEGLU, OUT_BF16_GEGLU_BWD = 5, 6   # include/encdiff_hip.h (pinned by test_gemm_fused_restate.py)
U = 2.0 ** -24                              # fp32 unit roundoff
GROUPS = 32

FUSED_ROUNDS = {
    # AGN (gemm_kernel<64,64,A_IM2COL_GN,...>)
    "agn_stats": "fp32 (mean, rstd) per (image, group) from fp32 sums of the bf16 x: var = E[x^2] - mean^2 "
                 "clamped at 0; recomputed by every workgroup, never stored",
    "agn_coef": "fp32 mul = rstd gamma (1 + scale), add = (beta - mean rstd gamma)(1 + scale) + shift",
    "agn_h": "z = x mul + add in fp32, SiLU in fp32 (__expf, v_rcp_f32); ROUNDED to bf16 in LDS (the MFMA "
             "operand), not stored; padding taps stay exactly zero",
    "agn_c": "fp32 accumulation, alpha, + bias + resid in fp32, rounded once; split-K: fp32 slabs, summed in "
             "split order, rounded once",
    "agn_gn_stats": "fp32 sum and sum of squares of the STORED bf16 c per 64-row segment and column",
    # LNA (gemm_kernel<64,64,A_ROWK_LN,...>)
    "lna_stats": "fp32 (mean, rstd) per row from fp32 sums of the bf16 row: one pass, var clamped at 0; not stored",
    "lna_h": "((x - mean) rstd) gamma + beta in fp32, ROUNDED to bf16 in LDS (the MFMA operand), not stored; "
             "the K tail and masked rows stay zero",
    "lna_c": "fp32 accumulation + bias + resid, rounded once",
    # ln_y (the epilogue of every ring tile)
    "ln_c": "fp32 accumulation, alpha, + bias + resid, rounded once; LayerNorm reads the ROUNDED row",
    "ln_stats": "fp32 (mean, rstd) of the bf16-rounded c row, two-pass (centred) variance",
    "ln_y": "(c - mean) rstd gamma + beta in fp32 from the rounded c, rounded once",
    # OUT_BF16_GEGLU
    "geglu_f": "fp32 accumulation, alpha, + bias, rounded once (both halves)",
    "geglu_y": "value * gelu(gate) in fp32 (erff) from the ROUNDED f, rounded once",
    # OUT_BF16_GEGLU_BWD
    "geglu_d": "alpha * (dy w) in fp32, ROUNDED to bf16 (as the unfused path stores it), not stored",
    "geglu_df": "(d gelu(g), d a gelu'(g)) in fp32 (erff, __expf) from the rounded d and the bf16 f; rounded once",
}


# ====================================================================== stages
def gelu(x):
    """F.gelu (erf form) in x's dtype"""
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def problem(M, Nn, K, a, b, *, a_mode=G.OPA_ROWK, b_mode=G.OPB_ROWK, conv=None, alpha=1.0, bias=None, resid=None):
    """gemm_restate.Problem of 2-D views (any device).  conv = (batch, h, w, cin, resample)."""
    fa, lda = G.flat(a)
    fb, ldb = G.flat(b)
    cv = None if conv is None else G.Conv(conv[0], conv[1], conv[2], conv[3], conv[4], a.stride(0))
    fr, ldr = G.flat(resid) if resid is not None else (None, 0)
    return G.Problem(M, Nn, K, a_mode, b_mode, G.OUT_BF16, fa, lda, fb, ldb, conv=cv, alpha=alpha, bias=bias,
                     resid=fr, ld_resid=ldr)


def with_a(P, h):
    """The same problem reading the dense operand h [rows][cols] (any dtype) in place of P.a"""
    Q = replace(P, a=h.reshape(-1))
    if P.conv is not None:
        Q.conv = replace(P.conv, ld_src=h.shape[1])
    else:
        Q.lda = h.shape[1]
    return Q


def linear_out(P, dtype=F64):
    """alpha A B (+ bias)(+ resid), [M][N]"""
    return G.result(P, dtype)["c"]


def carry(P, dh):
    """|dh| (an error bound of the A operand, [rows][cols]) through the contraction: |alpha| |dh| |B|"""
    Q = with_a(P, dh.double())
    Q = replace(Q, b=P.b.abs(), alpha=abs(P.alpha), bias=None, resid=None)
    return G.result(Q, F64)["c"]


# ---------------------------------------------------------------------- AGN
def agn_act(x, B, shw, gamma, beta, film, eps, silu, dtype=F64, stats=None):
    """SiLU?(GroupNorm32(x) (1 + scale) + shift) of the source rows x [B * shw][cin]: openaimodel_enc.py
    ResBlock in_layers (no FiLM) / out_layers (use_scale_shift_norm).  Returns (h, z)."""
    cin = x.shape[1]
    mean, rstd = stats if stats is not None else N.gn_stats_twopass(x, B, shw, GROUPS, eps, dtype)
    z, _ = N.gn_apply(x, B, shw, gamma, beta, mean, rstd, film=None if film is None else film[:, :2 * cin],
                      use_silu=False, dtype=dtype, centred=True)
    return (N.silu(z) if silu else z), z


def agn_stat_depth(cin, shw, nimg):
    """Serial-chain depth of the kernel's (image, group) sums: per-lane pixels, then lpi lanes, then cpg
    channels.  lpi = pixel lanes per image = (256 / (cin / 8)) / nimg, at least 1 (include/encdiff_hip.h
    says only 'fp32 sum / sum of squares'; the order is the kernel's and enters the bound, not the reference)."""
    np_ = 256 // (cin // 8)
    lanes = [max(np_ // n, 1) for n in range(1, nimg + 1)]     # a ragged or straddling tile reads fewer images
    return max(-(-shw // l) + l for l in lanes) + cin // GROUPS, lanes[-1]


def rstd_rel(t, dt, eps):
    """Relative error bound of rsqrtf(fl(t_k)) against t^-1/2 for a kernel value t_k = var_k + eps within dt
    of t; the kernel clamps var_k at 0, so t_k >= eps (1 - 2 U).  No first-order assumption (a constant
    group has t = eps and dt of the same size).  v_rsq_f32: 1 ulp = 2^-23."""
    lo = torch.maximum(t - dt, torch.full_like(t, eps * (1 - 2 * U)))
    up = torch.sqrt(t / lo)
    return torch.maximum(up - 1, 1 - torch.sqrt(t / (t + dt))) + 2.0 ** -23 * up


def onepass_slack(a1, e2, mean, var, eps, depth):
    """(dmean, rel_r) of one-pass fp32 statistics over n values with sum|x| / n = a1, sum x^2 / n = e2, the
    sums added along serial chains of `depth` (the serial-chain rule: depth U relative to the sum of
    absolute values):
      |dS1| <= depth U sum|x|,  |dS2| <= (depth + 1) U sum x^2   (the squares round once more)
      mean = fl(S1 fl(1 / n)), ex2 = fl(S2 fl(1 / n)): two more roundings each
      var = fl(ex2 - fl(mean mean)): |dvar| <= dex2 + 2 |mean| dmean + U mean^2 + U var
      rstd = rsqrtf(fl(var + eps)): rstd_rel(t, dvar + U t)"""
    dmean = depth * U * a1 + 2 * U * mean.abs()
    dex2 = (depth + 3) * U * e2
    dvar = dex2 + 2 * mean.abs() * dmean + dmean * dmean + U * mean * mean + U * var
    t = var + eps
    return dmean, rstd_rel(t, dvar + U * t, eps)


def agn_stat_slack(x, B, shw, gamma, beta, film, eps, silu, depth):
    """|kernel fp32 operand - true operand| per element of h, BEFORE the bf16 rounding.  The statistics by
    onepass_slack.  The kernel applies z = x mul + add with mul0 = fl(rstd gamma), add0 = fl(beta -
    fl(mean mul0)): in exact arithmetic on the kernel's own (mean, mul0) that is (x - mean) mul0 + beta, so
    the statistics enter as |x - mean| |mul0| rel_r + |mul0| dmean and the coefficient form adds its
    roundings relative to the LARGE terms |mean mul0|, |add0|, |x mul| (not to z: they cancel).  FiLM:
    sc = fl(1 + scale) scales both coefficients alike (U |z - shift|), mul = fl(mul0 sc), add = fl(fl(add0
    sc) + shift).  z = fl(fl(x mul) + add).  SiLU: |silu'| <= 1.1, silu_f's own error as
    resconv_restate.act_slack derives it (__expf, v_rcp_f32)."""
    cin = x.shape[1]
    cpg = cin // GROUPS
    v = N._bg(x.double(), B, shw, GROUPS)
    n = shw * cpg
    mean = v.mean(dim=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    dmean, rel_r = onepass_slack(v.abs().sum(dim=(1, 3)) / n, (v * v).sum(dim=(1, 3)) / n, mean, var, eps, depth)
    pc = lambda s: N._per_channel(s, cin)                        # [B][G] -> [B][1][C]
    ga, be = gamma.double(), beta.double()
    xv = x.double().reshape(B, shw, cin)
    mul0 = pc(1 / torch.sqrt(var + eps)) * ga
    add0 = be - pc(mean) * mul0
    dz = ((xv - pc(mean)).abs() * mul0.abs() * (pc(rel_r) + U) + mul0.abs() * pc(dmean) +
          U * ((pc(mean) * mul0).abs() + add0.abs()))
    mul, add = mul0, add0
    if film is not None:
        s1, sh = N.film_parts(film[:, :2 * cin], B, cin, F64)
        mul, add = mul0 * s1, add0 * s1 + sh
        dz = s1.abs() * dz + U * ((xv * mul + add - sh).abs() + (xv * mul).abs() + (add0 * s1).abs() + add.abs())
    z = xv * mul + add
    dz = dz + U * ((xv * mul).abs() + z.abs())
    if silu:
        dz = 1.1 * dz + R.silu(z).abs() * (2.0 ** -23 * (2 + z.abs()) + RC.SILU_REL_BASE)
    return dz.reshape(B * shw, cin)


def agn_cond(x, B, shw, eps):
    """the largest |mean| / std over the (image, group)s"""
    mean, rstd = N.gn_stats_twopass(x, B, shw, GROUPS, eps, F64)
    return (mean.abs() * rstd).max().item()


def agn_bound(I):
    """Reference and per-element bound of an AGN case (inputs namespace I, any device): ref (fp64), floor,
    rnd (the carried operand rounding), st (the carried statistics slack), tol."""
    P = I.P
    args = (I.x, I.B, I.shw, I.gamma, I.beta, I.film, I.eps, I.silu)
    h64, _ = agn_act(*args, dtype=F64)
    h32, _ = agn_act(*args, dtype=F32)
    ref64, ref32 = linear_out(with_a(P, h64), F64), linear_out(with_a(P, h32), F32)
    floor = R.floor_of(ref32, ref64)
    depth, _ = agn_stat_depth(I.cin, I.shw, I.nimg)
    st = agn_stat_slack(*args, depth)
    rnd = S.half_ulp(h64.abs() + st + R.floor_of(h32, h64))
    c_rnd, c_st = carry(P, rnd), carry(P, st)
    return NS(ref=ref64, ref32=ref32, floor=floor, rnd=c_rnd, st=c_st,
              tol=S.bf16_store_tol(ref64, c_rnd + c_st + floor), h=h64, cond=agn_cond(I.x, I.B, I.shw, I.eps))


# ---------------------------------------------------------------------- LNA
def lna_act(x, gamma, beta, eps, dtype=F64):
    """nn.LayerNorm over the K channels of the rows x [M][K] (attention.py norm1 / norm2 / norm3)"""
    return N.ln_fwd(x, gamma, beta, eps, dtype)[0]


def lna_stat_depth(K):
    """K / 32 vectors of 8 per lane (four lanes per row), then two shuffles"""
    return 8 * -(-K // 32) + 2


def lna_stat_slack(x, gamma, beta, eps, depth):
    """|kernel fp32 operand - true operand| per element before the bf16 rounding: the statistics by
    onepass_slack (n = K), then fl(fl(fl(fl(x - mean) rstd) gamma) + beta): four roundings."""
    v = x.double()
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    dmean, rel_r = onepass_slack(v.abs().mean(1, keepdim=True), (v * v).mean(1, keepdim=True), mean, var, eps, depth)
    rstd = 1 / torch.sqrt(var + eps)
    ga, be = gamma.double(), beta.double()
    xh = (v - mean) * rstd * ga
    return (rstd * ga).abs() * dmean + xh.abs() * (rel_r + 3 * U) + U * (xh + be).abs()


def lna_cond(x, eps):
    v = x.double()
    return (v.mean(1).abs() / torch.sqrt(v.var(1, unbiased=False) + eps)).max().item()


def lna_bound(I):
    P = I.P
    h64, h32 = lna_act(I.x, I.gamma, I.beta, I.eps, F64), lna_act(I.x, I.gamma, I.beta, I.eps, F32)
    ref64, ref32 = linear_out(with_a(P, h64), F64), linear_out(with_a(P, h32), F32)
    floor = R.floor_of(ref32, ref64)
    st = lna_stat_slack(I.x, I.gamma, I.beta, I.eps, lna_stat_depth(I.K))
    rnd = S.half_ulp(h64.abs() + st + R.floor_of(h32, h64))
    c_rnd, c_st = carry(P, rnd), carry(P, st)
    return NS(ref=ref64, ref32=ref32, floor=floor, rnd=c_rnd, st=c_st,
              tol=S.bf16_store_tol(ref64, c_rnd + c_st + floor), h=h64, cond=lna_cond(I.x, I.eps))


# ---------------------------------------------------------------------- ln_y
def ln_y_stage(c, gamma, beta, eps, dtype=F64):
    """(ln_y, ln_stats [M][2]) of the STORED rows c"""
    y, mean, rstd = N.ln_fwd(c, gamma, beta, eps, dtype)
    return y, torch.stack([mean, rstd], 1)


def stored_bound(ref64, ref32, slack=0.0):
    """(tol, floor) of a stored bf16 stage whose fp32 value is within slack + floor of ref64"""
    floor = R.floor_of(ref32, ref64)
    return S.bf16_store_tol(ref64, torch.as_tensor(slack, dtype=F64, device=ref64.device) + floor), floor


# ---------------------------------------------------------------------- GEGLU
def geglu_y(f, dtype=F64):
    """y = f[:, :I] * gelu(f[:, I:]) (attention.py GEGLU.forward) of the STORED f"""
    f = f.to(dtype)
    i = f.shape[1] // 2
    return f[:, :i] * gelu(f[:, i:])


def geglu_bwd(d, f, dtype=F64):
    """df = (d gelu(g) | d a gelu'(g)): the gradient of a gelu(g) for d(output) = d"""
    d, f = d.to(dtype), f.to(dtype)
    i = f.shape[1] // 2
    a, g = f[:, :i], f[:, i:]
    return torch.cat([d * gelu(g), d * a * gelu_grad(g)], 1)


def geglu_bwd_bound(P, f, exact=False):
    """df of the input-gradient problem P (d = alpha dy w, [M][inner]) and the saved f [M][2 inner].
    exact: d is an integer of magnitude <= 256, so bf16_round(d) is the identity and nothing is carried."""
    d64, d32 = linear_out(P, F64), linear_out(P, F32)
    ref64, ref32 = geglu_bwd(d64, f, F64), geglu_bwd(d32, f, F32)
    floor = R.floor_of(ref32, ref64)
    car = torch.zeros_like(ref64)
    if not exact:
        hd = S.half_ulp(d64.abs() + R.floor_of(d32, d64))
        i = f.shape[1] // 2
        g = f[:, i:].double()
        car = torch.cat([hd * gelu(g).abs(), hd * (f[:, :i].double() * gelu_grad(g)).abs()], 1)
    return NS(ref=ref64, ref32=ref32, floor=floor, rnd=car, tol=S.bf16_store_tol(ref64, car + floor), d=d64)


# ====================================================================== the shared case tables
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# AGN: name -> dict.  (B, h, w) the OUTPUT grid; up2: the source is (h / 2, w / 2).  ms: |mean| / std of the
# groups (cases with ms <= 4 must keep the statistics slack below 1/8 of the rounding term).
def _agn(B, h, w, cin, cout, up2=False, film=False, silu=True, eps=1e-5, bias=True, resid=False, gn=False,
         split=1, fold=False, ms=2.0, const=False, ld_extra=8):
    return dict(B=B, h=h, w=w, cin=cin, cout=cout, up2=up2, film=film, silu=silu, eps=eps, bias=bias, resid=resid,
                gn=gn, split=split, fold=fold, ms=ms, const=const, ld_extra=ld_extra)


AGN_CASES = {
    "b6-4x4-c64": _agn(6, 4, 4, 64, 64, film=True),                       # 4 images per tile, tap-uniform
    "b3-2x2-c32": _agn(3, 2, 2, 32, 64, film=True, eps=1e-6),             # cpg 1, k-tile spans two taps, K tail
    "b2-8x8-c96": _agn(2, 8, 8, 96, 72, film=True, resid=True),           # nv 12: idle lanes; ragged column tile
    "b20-1x1-c64": _agn(20, 1, 1, 64, 64, film=True, silu=False),          # centre tap only, ragged last tile
    "b2-6x6-c64": _agn(2, 6, 6, 64, 64, film=True),                       # tiles straddle images, ragged M
    "b2-16x16-c64": _agn(2, 16, 16, 64, 64, film=True, gn=True),          # a tile is four rows of one image
    "b70-1x1-c64": _agn(70, 1, 1, 64, 64),                                # 64 images per tile: gst fills the ring
    "b16-2x2-c512": _agn(16, 2, 2, 512, 64, film=True),                   # np 4 < nimg 16: lpi 1, four passes
    "b4-4x4-c1024": _agn(4, 4, 4, 1024, 64),                              # np 2, two passes
    "b5-3x5-c32": _agn(5, 3, 5, 32, 72, film=True, silu=False, bias=False),  # unaligned straddle, nimg varies
    "b1-8x8-c64": _agn(1, 8, 8, 64, 64, resid=True, gn=True),             # B = 1
    "b3-6x6-c32": _agn(3, 6, 6, 32, 64, eps=1e-6),
    "b8-up4x4-c64": _agn(8, 4, 4, 64, 64, up2=True, film=True),           # UP2 2x2 -> 4x4, several images per tile
    "b2-up16x16-c32": _agn(2, 16, 16, 32, 64, up2=True),                  # UP2 8x8 -> 16x16
    "b4-8x8-c128-split2": _agn(4, 8, 8, 128, 72, film=True, split=2, resid=True),
    "b4-8x8-c128-fold2": _agn(4, 8, 8, 128, 72, film=True, split=2, fold=True, resid=True),
    "b4-4x4-c64-const": _agn(4, 4, 4, 64, 64, film=True, const=True),      # image 1 constant: var 0, the clamp
    "b4-4x4-c64-ms16": _agn(4, 4, 4, 64, 64, film=True, ms=16.0),          # conditioning: exempt from the 1/8 cap
}
# the cases the mutation checks of test_gemm_fused_restate.py run on
AGN_MUT_CASES = ["b6-4x4-c64", "b3-2x2-c32", "b2-8x8-c96", "b20-1x1-c64", "b2-6x6-c64", "b2-16x16-c64"]


def agn_tile_images(B, h, w):
    """The largest number of images one 64-row tile reads"""
    hw, M = h * w, B * h * w
    return max(min(m0 + 63, M - 1) // hw - m0 // hw + 1 for m0 in range(0, M, 64))


def agn_inputs(name, put=lambda k, t: t, seed=None):
    """The inputs of an AGN case.  put(kind, host tensor) places one: kind 'x' / 'w' / 'resid' (bf16 2-D),
    'film' (fp32 2-D), 'vec' (fp32 1-D).  Per-(image, group) means and scales differ by factors of 2-4."""
    c = AGN_CASES[name]
    g = _g(1000 + sorted(AGN_CASES).index(name) if seed is None else seed)
    B, h, w, cin, cout = c["B"], c["h"], c["w"], c["cin"], c["cout"]
    hs, ws = (h // 2, w // 2) if c["up2"] else (h, w)
    shw, cpg = hs * ws, cin // GROUPS
    scale = 0.5 * 2.0 ** torch.randint(0, 3, (B, 1, GROUPS, 1), generator=g)
    sign = 2.0 * torch.randint(0, 2, (B, 1, GROUPS, 1), generator=g) - 1
    mean = sign * scale * c["ms"] * (0.25 + 0.75 * torch.rand(B, 1, GROUPS, 1, generator=g))
    if c["ms"] > 4:
        mean = sign * scale * c["ms"]
    x = mean + scale * _randn(g, B, shw, GROUPS, cpg)
    if c["const"]:
        x[1] = 0.75
    x = x.reshape(B * shw, cin)
    gamma = 1 + 0.3 * _randn(g, cin)
    beta = 0.3 * _randn(g, cin)
    film = torch.cat([0.5 * _randn(g, B, cin), 0.5 * _randn(g, B, cin), torch.full((B, 8), float("nan"))], 1) \
        if c["film"] else None
    wt = _randn(g, cout, 9 * cin) * (9 * cin) ** -0.5
    bias = 0.2 * _randn(g, cout) if c["bias"] else None
    resid = _randn(g, B * h * w, cout) if c["resid"] else None
    I = NS(name=name, B=B, hh=h, ww=w, cin=cin, cout=cout, shw=shw, eps=c["eps"], silu=c["silu"], case=c,
           M=B * h * w, K=9 * cin, nimg=agn_tile_images(B, h, w), resample=G.UP2 if c["up2"] else G.NONE)
    I.x = put("x", x.to(BF16))
    I.w = put("w", wt.to(BF16))
    I.gamma, I.beta = put("vec", gamma), put("vec", beta)
    I.film = None if film is None else put("film", film)[:, :2 * cin]
    I.bias = None if bias is None else put("vec", bias)
    I.resid = None if resid is None else put("resid", resid.to(BF16))
    I.P = problem(I.M, cout, I.K, I.x, I.w, a_mode=G.OPA_IM2COL, conv=(B, h, w, cin, I.resample), bias=I.bias,
                  resid=I.resid)
    return I


# LNA: (M, K, N), resid, ms, constant row
def _lna(M, K, Nn, resid=False, bias=True, ms=1.0, const=False, eps=1e-5):
    return dict(M=M, K=K, N=Nn, resid=resid, bias=bias, ms=ms, const=const, eps=eps)


LNA_CASES = {
    "m100-k8-n72": _lna(100, 8, 72),                     # lanes q = 1..3 without a vector
    "m70-k72-n64": _lna(70, 72, 64, resid=True),         # tail of the 32-stride loop and of the 64-wide k-tile
    "m65-k256-n136": _lna(65, 256, 136),
    "m1-k1024-n64": _lna(1, 1024, 64, bias=False),       # the LDS maximum
    "m64-k520-n8": _lna(64, 520, 8, resid=True),
    "m65-k72-n64-const": _lna(65, 72, 64, const=True),   # row 3 constant: var 0, the clamp
    "m65-k256-n64-ms16": _lna(65, 256, 64, ms=16.0),     # conditioning: exempt from the 1/8 cap
}
LNA_MUT_CASES = ["m100-k8-n72", "m70-k72-n64", "m65-k256-n136", "m1-k1024-n64", "m64-k520-n8"]


def row_inputs(g, M, K, ms):
    """Rows whose means and scales differ by factors of 2-4"""
    scale = 0.5 * 2.0 ** torch.randint(0, 3, (M, 1), generator=g)
    sign = 2.0 * torch.randint(0, 2, (M, 1), generator=g) - 1
    mean = sign * scale * ms * ((0.25 + 0.75 * torch.rand(M, 1, generator=g)) if ms <= 4 else 1.0)
    return mean + scale * _randn(g, M, K)


def lna_inputs(name, put=lambda k, t: t):
    c = LNA_CASES[name]
    g = _g(2000 + sorted(LNA_CASES).index(name))
    M, K, Nn = c["M"], c["K"], c["N"]
    x = row_inputs(g, M, K, c["ms"])
    if c["const"]:
        x[min(3, M - 1)] = -1.5
    I = NS(name=name, M=M, K=K, N=Nn, eps=c["eps"], case=c)
    I.x = put("x", x.to(BF16))
    I.w = put("w", (_randn(g, Nn, K) * K ** -0.5).to(BF16))
    I.gamma, I.beta = put("vec", 1 + 0.3 * _randn(g, K)), put("vec", 0.3 * _randn(g, K))
    I.bias = put("vec", 0.2 * _randn(g, Nn)) if c["bias"] else None
    I.resid = put("resid", _randn(g, M, Nn).to(BF16)) if c["resid"] else None
    I.P = problem(M, Nn, K, I.x, I.w, bias=I.bias, resid=I.resid)
    return I


# ln_y: (tile, M, N, K, way): way = "vec" or the way onto the scalar epilogue
def _lny(tile, M, Nn, K, way="vec", alpha=1.0, bias=True, resid=False, exact=False, ld_y_extra=0):
    return dict(tile=tile, M=M, N=Nn, K=K, way=way, alpha=alpha, bias=bias, resid=resid, exact=exact,
                ld_y_extra=ld_y_extra)


LNY_CASES = {
    "t1-m130-n128": _lny(1, 130, 128, 72, resid=True),
    "t1-m65-n64": _lny(1, 65, 64, 200),                          # N 64 on a 128-wide tile
    "t2-m130-n64": _lny(2, 130, 64, 8, alpha=0.5),
    "t2-m1-n8": _lny(2, 1, 8, 72),
    "t3-m65-n128": _lny(3, 65, 128, 200, ld_y_extra=8),
    "t3-m130-n24": _lny(3, 130, 24, 72, resid=True),
    "t4-m65-n64": _lny(4, 65, 64, 72, resid=True, ld_y_extra=16),
    "t4-m1-n8": _lny(4, 1, 8, 8),
    "t5-m130-n24": _lny(5, 130, 24, 200),
    "t6-m65-n128": _lny(6, 65, 128, 72, alpha=0.5),
    "t7-m130-n64": _lny(7, 130, 64, 200, resid=True),
    "t8-m65-n64": _lny(8, 65, 64, 72),                           # N 64 on a 128-wide tile, KB 128
    "t9-m65-n8": _lny(9, 65, 8, 72),
    "t10-m130-n64": _lny(10, 130, 64, 8),
    "t4-m65-n64-ldc": _lny(4, 65, 64, 72, way="ldc", resid=True),
    "t3-m65-n128-bias": _lny(3, 65, 128, 72, way="bias_misaligned"),
    "t2-m130-n64-resid": _lny(2, 130, 64, 72, way="resid_misaligned", resid=True),
    "t4-m65-n24-ldresid": _lny(4, 65, 24, 72, way="ld_resid", resid=True),
    "t4-m65-n64-exact": _lny(4, 65, 64, 72, resid=True, exact=True),
    "t1-m130-n128-exact": _lny(1, 130, 128, 200, alpha=0.5, exact=True),
    "t3-m65-n64-exact-ldc": _lny(3, 65, 64, 72, way="ldc", exact=True),
}
LNY_MUT_CASES = ["t1-m65-n64", "t2-m1-n8", "t4-m65-n64", "t3-m65-n128", "t9-m65-n8"]


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def lny_inputs(name, put=lambda k, t: t):
    """put kinds as agn_inputs plus 'bias' (the fp32 bias, which one way misaligns) and 'resid_way'"""
    c = LNY_CASES[name]
    g = _g(3000 + sorted(LNY_CASES).index(name))
    M, Nn, K = c["M"], c["N"], c["K"]
    I = NS(name=name, M=M, N=Nn, K=K, eps=1e-5, case=c, tile=c["tile"], alpha=c["alpha"])
    if c["exact"]:
        x, w = _ints(g, M, K), _ints(g, Nn, K)
        bias = _ints(g, Nn) if c["bias"] else None
        resid = _ints(g, M, Nn) if c["resid"] else None
    else:
        x, w = row_inputs(g, M, K, 1.0), _randn(g, Nn, K) * K ** -0.5
        bias = 0.5 * _randn(g, Nn) if c["bias"] else None
        resid = row_inputs(g, M, Nn, 1.0) if c["resid"] else None
    I.x, I.w = put("x", x.to(BF16)), put("w", w.to(BF16))
    I.gamma, I.beta = put("vec", 1 + 0.3 * _randn(g, Nn)), put("vec", 0.3 * _randn(g, Nn))
    I.bias = None if bias is None else put("bias", bias)
    I.resid = None if resid is None else put("resid_way", resid.to(BF16))
    I.P = problem(M, Nn, K, I.x, I.w, alpha=c["alpha"], bias=I.bias, resid=I.resid)
    return I


# GEGLU forward: (tile, M, N = 2 inner, K)
def _gg(tile, M, Nn, K, alpha=1.0, bias=True, exact=False):
    return dict(tile=tile, M=M, N=Nn, K=K, alpha=alpha, bias=bias, exact=exact)


GEGLU_CASES = {
    "t1-m130-n128": _gg(1, 130, 128, 72),               # one column tile holds both halves
    "t1-m65-n256": _gg(1, 65, 256, 200, alpha=0.5),
    "t2-m130-n128": _gg(2, 130, 128, 8, bias=False),
    "t2-m1-n256": _gg(2, 1, 256, 72),
    "t3-m65-n384": _gg(3, 65, 384, 72),
    "t4-m65-n128": _gg(4, 65, 128, 200),
    "t4-m130-n256": _gg(4, 130, 256, 72, alpha=0.5, bias=False),
    "t5-m65-n256": _gg(5, 65, 256, 200),
    "t6-m130-n384": _gg(6, 130, 384, 72),
    "t7-m65-n128": _gg(7, 65, 128, 200),
    "t8-m1-n256": _gg(8, 1, 256, 72),
    "t9-m65-n128": _gg(9, 65, 128, 8),
    "t10-m130-n256": _gg(10, 130, 256, 72),
    "t4-m65-n256-exact": _gg(4, 65, 256, 72, exact=True),
    "t1-m130-n384-exact": _gg(1, 130, 384, 200, alpha=0.5, exact=True),
    "t3-m65-n128-exact": _gg(3, 65, 128, 72, exact=True),
}
GEGLU_MUT_CASES = ["t1-m65-n256", "t4-m130-n256", "t3-m65-n384", "t4-m65-n128", "t5-m65-n256"]


def geglu_inputs(name, put=lambda k, t: t):
    c = GEGLU_CASES[name]
    g = _g(4000 + sorted(GEGLU_CASES).index(name))
    M, Nn, K = c["M"], c["N"], c["K"]
    I = NS(name=name, M=M, N=Nn, K=K, case=c, tile=c["tile"], alpha=c["alpha"])
    if c["exact"]:
        x, w, bias = _ints(g, M, K), _ints(g, Nn, K), (_ints(g, Nn) if c["bias"] else None)
    else:
        x, w = _randn(g, M, K), _randn(g, Nn, K) * (2.0 / K) ** 0.5
        bias = 0.5 * _randn(g, Nn) + torch.linspace(-1, 1, Nn) if c["bias"] else None
    I.x, I.w = put("x", x.to(BF16)), put("w", w.to(BF16))
    I.bias = None if bias is None else put("vec", bias)
    I.P = problem(M, Nn, K, I.x, I.w, alpha=c["alpha"], bias=I.bias)
    return I


# GEGLU backward: the input gradient d [M][Ni] = alpha dy [M][K] w [K][Ni] (ROWK x ROWN), f [M][2 Ni]
def _gb(tile, M, Ni, K, exact=False, pair=False):
    return dict(tile=tile, M=M, N=Ni, K=K, exact=exact, pair=pair)


GEGLU_BWD_CASES = {
    "t1-m130-n200": _gb(1, 130, 200, 72),
    "t2-m65-n72": _gb(2, 65, 72, 256),
    "t3-m1-n128": _gb(3, 1, 128, 8),
    "t4-m65-n8": _gb(4, 65, 8, 72),
    "t4-m130-n200": _gb(4, 130, 200, 256),
    "t5-m65-n72": _gb(5, 65, 72, 72),
    "t6-m130-n128": _gb(6, 130, 128, 8),
    "t7-m65-n200": _gb(7, 65, 200, 256),
    "t8-m1-n72": _gb(8, 1, 72, 72),
    "t9-m65-n128": _gb(9, 65, 128, 72),
    "t10-m130-n8": _gb(10, 130, 8, 256),
    "t4-m65-n72-exact": _gb(4, 65, 72, 256, exact=True),
    "t1-m130-n128-exact": _gb(1, 130, 128, 72, exact=True),
    "t3-m65-n200-exact": _gb(3, 65, 200, 8, exact=True),
    "t4-m64-n128-pair": _gb(4, 64, 128, 64, pair=True),
    "t4-m128-n64-pair-exact": _gb(4, 128, 64, 64, exact=True, pair=True),
}
GEGLU_BWD_MUT_CASES = ["t1-m130-n200", "t2-m65-n72", "t4-m130-n200", "t7-m65-n200", "t9-m65-n128"]
GATE_PLANTS = [0.0, -0.0, 6.0, -6.0, 30.0, -30.0]


def geglu_bwd_inputs(name, put=lambda k, t: t):
    """dy [M][K], w [K][Ni] (the next layer's weight, [out][in]), f [M][2 Ni] with the gate values
    0, -0, +-6, +-30 planted at the head of the gate half of the first and the last row"""
    c = GEGLU_BWD_CASES[name]
    g = _g(5000 + sorted(GEGLU_BWD_CASES).index(name))
    M, Ni, K = c["M"], c["N"], c["K"]
    I = NS(name=name, M=M, N=Ni, K=K, case=c, tile=c["tile"], exact=c["exact"])
    if c["exact"]:   # operands in {-1, 0, 1}, K <= 256: d is an integer of magnitude <= 256
        dy, w = _ints(g, M, K, lo=-1, hi=1), _ints(g, K, Ni, lo=-1, hi=1)
    else:
        dy, w = _randn(g, M, K), _randn(g, K, Ni) * K ** -0.5
    f = _randn(g, M, 2 * Ni) * 1.5
    k = min(len(GATE_PLANTS), Ni)
    f[0, Ni:Ni + k] = torch.tensor(GATE_PLANTS[:k])
    f[M - 1, 2 * Ni - k:] = torch.tensor(GATE_PLANTS[:k])
    I.dy, I.w, I.f = put("x", dy.to(BF16)), put("w", w.to(BF16)), put("f", f.to(BF16))
    I.P = problem(M, Ni, K, I.dy, I.w, b_mode=G.OPB_ROWN)
    return I


# ====================================================================== kernel models (fp32, the kernels' order)
# What the bounds must admit: fp32 one-pass statistics added in the kernels' order, the operand rounded
# to bf16, fp32 accumulation, a bf16 store.  `mutate` plants one of the mistakes the bounds must reject.
def _rb(t):
    return t.to(BF16).to(F32)


def _lin32(P, h):
    """fp32 accumulation of the bf16 operand h through P, bf16 store"""
    return _rb(linear_out(with_a(P, h), F32))


def agn_model(I, mutate=None):
    B, shw, cin = I.B, I.shw, I.cin
    cpg = cin // GROUPS
    _, lpi = agn_stat_depth(cin, shw, I.nimg)
    x = I.x.to(F32).reshape(B, shw, cin)
    s, q = torch.zeros(B, lpi, cin), torch.zeros(B, lpi, cin)
    for px in range(shw):           # lane px % lpi takes its pixels in order
        s[:, px % lpi] += x[:, px]
        q[:, px % lpi] += x[:, px] * x[:, px]
    a, b = torch.zeros(B, cin), torch.zeros(B, cin)
    for r in range(lpi):            # lanes in order
        a, b = a + s[:, r], b + q[:, r]
    ga, gq = torch.zeros(B, GROUPS), torch.zeros(B, GROUPS)
    for c in range(cpg):            # channels of the group in order
        ga, gq = ga + a.reshape(B, GROUPS, cpg)[:, :, c], gq + b.reshape(B, GROUPS, cpg)[:, :, c]
    n = shw * cpg
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(n), dtype=F32)
    mean = ga * inv
    var = (gq * inv - mean * mean).clamp_min(0)
    if mutate == "unbiased":
        var = var * (n / max(n - 1, 1))
    rstd = torch.rsqrt(var + I.eps)
    if mutate == "neighbour":       # the coefficient rows of the neighbouring image
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    if mutate == "group":           # group index off by one
        mean, rstd = mean.roll(1, 1), rstd.roll(1, 1)
    pc = lambda t: N._per_channel(t, cin)
    mul = pc(rstd) * I.gamma.to(F32)
    add = I.beta.to(F32) - pc(mean) * mul
    if I.film is not None:
        sc, sh = I.film[:, :cin].to(F32).reshape(B, 1, cin), I.film[:, cin:2 * cin].to(F32).reshape(B, 1, cin)
        if mutate == "film_swap":
            sc, sh = sh, sc
        s1 = sc if mutate == "no_one_plus" else 1 + sc
        mul = mul * s1
        add = add * s1 + sh
    z = x * mul + add
    if I.silu and mutate != "no_silu":
        z = z * (1 / (1 + torch.exp(-z)))
    return _lin32(I.P, _rb(z).reshape(B * shw, cin))


AGN_MUTATIONS = ["neighbour", "group", "film_swap", "no_one_plus", "no_silu", "unbiased"]


def lna_model(I, mutate=None):
    M, K = I.M, I.K
    x = I.x.to(F32)
    sa, sq = torch.zeros(M, 4), torch.zeros(M, 4)
    for k0 in range(0, K, 8):       # lane (k0 / 8) % 4 adds its vectors of 8 element by element
        lane = (k0 // 8) % 4
        for e in range(8):
            sa[:, lane] += x[:, k0 + e]
            sq[:, lane] += x[:, k0 + e] * x[:, k0 + e]
    s1 = (sa[:, 0] + sa[:, 1]) + (sa[:, 2] + sa[:, 3])
    s2 = (sq[:, 0] + sq[:, 1]) + (sq[:, 2] + sq[:, 3])
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(K), dtype=F32)
    mean = s1 * inv
    var = (s2 * inv - mean * mean).clamp_min(0)
    if mutate == "unbiased":
        var = var * (K / (K - 1))
    rstd = torch.rsqrt(var + I.eps)
    if mutate == "neighbour":
        mean, rstd = mean.roll(1), rstd.roll(1)
    ga, be = I.gamma.to(F32), I.beta.to(F32)
    if mutate == "gb_shift8":
        ga, be = ga.roll(8), be.roll(8)
    h = _rb((x - mean[:, None]) * rstd[:, None] * ga + be)
    P = I.P
    if mutate == "tail":
        # the zero-staged K tail of the last 64-wide k-tile normalised as well: (0 - mean) rstd gamma + beta
        # with the gamma / beta LDS slots behind K, which nothing ever wrote (modelled as NaN); B is zero
        # there, so only a non-finite product shows
        Kp = -(-K // 64) * 64
        if Kp > K:
            tail = (0 - mean[:, None]) * rstd[:, None] * torch.full((Kp - K,), float("nan")) + float("nan")
            hp = torch.cat([h, tail], 1)
            wp = torch.cat([G.dense_b(P, F32), torch.zeros(Kp - K, P.N)], 0)
            c = (hp @ wp) * P.alpha
            c = c + (P.bias.to(F32) if P.bias is not None else 0)
            if P.resid is not None:
                c = c + G._rows(P.resid, P.ld_resid, M, P.N, F32)
            return _rb(c)
    return _lin32(P, h)


LNA_MUTATIONS = ["neighbour", "gb_shift8", "unbiased", "tail"]


def lny_model(I, c, mutate=None, bn=None):
    """ln_y from the STORED c [M][N] (bf16): two-pass fp32 statistics; bn: the tile width"""
    v = c.to(F32)
    Nn = v.shape[1]
    mean = v.sum(1, keepdim=True) / Nn
    div = Nn
    if mutate == "div_bn":
        div = bn
    if mutate == "unbiased":
        div = Nn - 1
    rstd = torch.rsqrt(((v - mean) ** 2).sum(1, keepdim=True) / div + I.eps)
    if mutate == "neighbour":
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    ga, be = I.gamma.to(F32), I.beta.to(F32)
    if mutate == "gb_shift8":
        ga, be = ga.roll(8), be.roll(8)
    return _rb((v - mean) * rstd * ga + be), torch.cat([mean, rstd], 1)


LNY_MUTATIONS = ["div_bn", "neighbour", "gb_shift8", "unbiased"]


def geglu_model(I, mutate=None, bn=64):
    """(f, y) of the forward: f = bf16(alpha x w^T + bias), y = bf16(value * gelu(gate)) from the rounded f"""
    P = I.P
    acc = (G.dense_a(P, F32) @ G.dense_b(P, F32)) * P.alpha
    i = P.N // 2
    bias = P.bias.to(F32) if P.bias is not None else torch.zeros(P.N)
    if mutate == "gate_bias":       # the gate's bias read at the value's column
        bias = torch.cat([bias[:i], bias[:i]])
    f = _rb(acc + bias)
    a, g = f[:, :i], f[:, i:]
    if mutate == "halves":
        a, g = g, a
    if mutate == "next_tile":       # gcol with the wrong by: the gate of the next column tile
        g = g.roll(-(bn // 2), 1)
    return f, _rb(a * gelu(g))


GEGLU_MUTATIONS = ["halves", "next_tile", "gate_bias"]


def geglu_bwd_model(I, mutate=None):
    P = I.P
    d = _rb((G.dense_a(P, F32) @ G.dense_b(P, F32)) * P.alpha)
    f = I.f.to(F32)
    i = P.N
    a, g = f[:, :i], f[:, i:]
    if mutate == "gate_col":        # the gate read at column col instead of N + col
        g = a
    gg = 0.5 * (1 + torch.erf(g * 0.7071067811865476)) if mutate == "no_pdf" else gelu_grad(g)
    dg = d * gg if mutate == "no_a" else d * a * gg
    return _rb(torch.cat([d * gelu(g), dg], 1))


GEGLU_BWD_MUTATIONS = ["no_a", "no_pdf", "gate_col"]


def exceeds(out, ref, tol):
    """Fraction of the elements outside the bound (a NaN is outside)"""
    return (~((out.double() - ref).abs() <= tol)).double().mean().item()
