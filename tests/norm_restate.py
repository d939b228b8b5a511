"""Pure-torch restatements of the normalisation kernels (csrc/norm.hip and the four norm kernels of
csrc/fp32.hip), written from include/encdiff_hip.h's description of the entry points and the
formulas of GroupNorm / FiLM / SiLU / LayerNorm, not from the kernels' loops.
tests/test_gpu_norm.py compares the HIP kernels with them; tests/test_norm_restate.py checks the
restatements themselves on the CPU (against torch autograd in fp64).

Everything takes a `dtype`: evaluated in fp64 it is the reference, in fp32 the "torch fp32
evaluation" whose distance from fp64 sets the additive floor of the comparison rules
(tests/elementwise_restate.py).  Activations are rows [B * HW][C] (NHWC), statistics [B][G] pairs.

Also here: a Python copy of the dispatch arithmetic of norm.hip (gn_slice and what follows from
it), so that every GPU case can assert which kernel path it reaches.
"""
import torch

import elementwise_restate as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

DOWN2, UP2 = 1, 2  # EncdiffResample values of dy_resample / resid_resample (checked against _lib on the GPU)


# ------------------------------------------------------------------ dispatch (a copy of norm.hip's)
GN_THREADS = 256
GN_TILE = 1024      # backward LDS tile, 16-byte vectors
GN_TILE_FWD = 6144  # forward LDS tile
GN_BWD_U = 4        # backward rows per thread and batch
GN_MIN_SLICE = 8192


def gn_slice(C, HW, cpg, batch, min_slice=GN_MIN_SLICE):
    """Channel-slice width: the narrowest multiple of lcm(8, cpg) dividing C whose slice holds
    >= min_el elements, else C.  min_el: min_slice (a quarter below 64 images), halved / quartered /
    an eighth below 256 / 64 / 16 pixels."""
    unit = 8
    while unit % cpg:
        unit += 8
    shrink = 1 if HW >= 256 else (2 if HW >= 64 else (4 if HW >= 16 else 8))
    min_el = (min_slice if batch >= 64 else min_slice // 4) // shrink
    for w in range(unit, C, unit):
        if C % w == 0 and w * HW >= min_el:
            return w
    return C


class GnPath:
    """What encdiff_groupnorm_fwd / _bwd do with (C, HW, B, groups): slice, lanes and kernel path."""

    def __init__(self, C, HW, B, groups=32, in_stats=False, ld_in_stats=None, slab=False):
        self.ok = C % 8 == 0 and groups > 0 and C % groups == 0
        if not self.ok:
            return
        cpg = C // groups
        self.cpg = cpg
        self.cs = cs = gn_slice(C, HW, cpg, B)
        self.ok = cs <= 512 and cs // cpg <= 64
        self.nvc = nvc = cs // 8
        self.np = np_ = GN_THREADS // nvc
        self.pow2 = nvc & (nvc - 1) == 0
        self.idle = GN_THREADS - nvc * np_            # threads without a pixel lane
        self.grid = B * (C // cs)
        # butterfly of slice_partials: levels = min(3, log2(64 / nvc)); nval = 8 >> levels
        lv, off = 0, nvc
        while self.pow2 and lv < 3 and off < 64:
            lv, off = lv + 1, off * 2
        self.nval = (8 >> lv) if self.pow2 else None
        self.red_rows = (GN_THREADS // nvc if nvc >= 64 else 4) if self.pow2 else np_
        # forward
        st_ok = in_stats and HW % 64 == 0 and (C if ld_in_stats is None else ld_in_stats) >= C
        if st_ok and HW >= 1024 and C <= 512 and groups <= 64 and GN_THREADS % (C >> 3) == 0:
            self.fwd = "group_apply"
        elif st_ok and (HW // 64) * cs <= 2048:
            self.fwd = "stats"
        else:
            self.fwd = "self"
        self.fwd_tiled = nvc * HW <= GN_TILE_FWD
        # backward
        self.one = (not slab) and HW <= GN_BWD_U * np_
        self.bwd_tiled = (not self.one) and nvc * HW <= GN_TILE
        self.last_batch_partial = HW % (GN_BWD_U * np_) != 0


def ln_rpb(C):
    """Rows per block-iteration of the bf16 LayerNorm kernels (C / 8 lanes per row, 256 threads)."""
    return 256 // (C // 8)


LN_PARTS = 256
LN_FWD_GRID_CAP = 4096


# ------------------------------------------------------------------ small pieces
def silu(z):
    return R.silu(z)


def silu_grad(z):
    return R.silu_grad(z)


def _bg(t, B, HW, G):
    """rows [B*HW][C] -> [B][HW][G][cpg]"""
    return t.reshape(B, HW, G, -1)


def _per_channel(st, C):
    """[B][G] -> [B][1][C]"""
    B, G = st.shape
    return st.repeat_interleave(C // G, dim=1).reshape(B, 1, C)


def film_parts(film, B, C, dtype):
    """film [B][>= 2C] -> (1 + scale, shift) as [B][1][C]; ones / zeros without FiLM."""
    if film is None:
        return None, None
    f = film.to(dtype)
    return (1 + f[:, :C]).reshape(B, 1, C), f[:, C:2 * C].reshape(B, 1, C)


# ------------------------------------------------------------------ GroupNorm forward
def gn_stats_onepass(x, B, HW, G, eps, dtype=F64):
    """(mean, rstd) [B][G] the way the bf16 kernels form them: one pass, var = E[x^2] - mean^2
    (clamped at 0), both moments summed in `dtype`."""
    v = _bg(x.to(dtype), B, HW, G)
    n = v.shape[1] * v.shape[3]
    mean = v.sum(dim=(1, 3)) / n
    ex2 = (v * v).sum(dim=(1, 3)) / n
    var = (ex2 - mean * mean).clamp_min(0)
    return mean, 1 / torch.sqrt(var + eps)


def gn_stats_twopass(x, B, HW, G, eps, dtype=F64):
    """(mean, rstd) with the centred variance (the fp32 kernels; F.group_norm)."""
    v = _bg(x.to(dtype), B, HW, G)
    mean = v.mean(dim=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, 1 / torch.sqrt(var + eps)


def segment_stats(x, B, HW, ld=None, pad=float("nan")):
    """in_stats as x's producer GEMM writes them: per 64-row segment the channel sums (k = 0) and
    sums of squares (k = 1), element [(2 (b nseg + sg) + k) ld + c]; from x in fp64, rounded to
    fp32.  Columns C.. (ld > C) hold `pad`."""
    rows, C = x.shape
    assert HW % 64 == 0 and rows == B * HW
    ld = C if ld is None else ld
    nseg = HW // 64
    v = x.double().reshape(B * nseg, 64, C)
    out = torch.full((2 * B * nseg, ld), pad, dtype=F32, device=x.device)
    out[0::2, :C] = v.sum(1).to(F32)
    out[1::2, :C] = (v * v).sum(1).to(F32)
    return out


def gn_stats_from_segments(in_stats, B, HW, C, G, eps, dtype=F64):
    """(mean, rstd) [B][G] from segment sums (one-pass form; the only form they allow)."""
    nseg = HW // 64
    s = in_stats[:, :C].to(dtype).reshape(B, nseg, 2, G, C // G)
    n = HW * (C // G)
    mean = s[:, :, 0].sum(dim=(1, 3)) / n
    ex2 = s[:, :, 1].sum(dim=(1, 3)) / n
    var = (ex2 - mean * mean).clamp_min(0)
    return mean, 1 / torch.sqrt(var + eps)


def gn_apply(x, B, HW, gamma, beta, mean, rstd, film=None, use_silu=False, dtype=F64, centred=False):
    """From given statistics: y = x mul + add with mul = rstd gamma (1 + scale), add = (beta - mean
    rstd gamma)(1 + scale) + shift (the bf16 kernels' form); centred (the fp32 kernels' form):
    ((x - mean) rstd gamma + beta)(1 + scale) + shift.  Returns (y or silu(y), silu'(z) or None)."""
    C = x.shape[1]
    v = x.to(dtype).reshape(B, HW, C)
    s1, sh = film_parts(film, B, C, dtype)
    if centred:
        z = (v - _per_channel(mean.to(dtype), C)) * _per_channel(rstd.to(dtype), C) * gamma.to(dtype) + beta.to(dtype)
        if film is not None:
            z = z * s1 + sh
    else:
        mul = _per_channel(rstd.to(dtype), C) * gamma.to(dtype)
        add = beta.to(dtype) - _per_channel(mean.to(dtype), C) * mul
        if film is not None:
            mul = mul * s1
            add = add * s1 + sh
        z = v * mul + add
    z = z.reshape(B * HW, C)
    if use_silu:
        return silu(z), silu_grad(z)
    return z, None


# ------------------------------------------------------------------ resample adjoints
def resample_adjoint(t, mode, B, h, w, dtype=F64):
    """t at the resolution of a 2x resample FOLLOWING an (h, w) tensor -> its adjoint at (h, w).
    DOWN2 (avg-pool after): t is (h/2, w/2), 0.25 t[y/2][x/2].  UP2 (nearest after): t is (2h, 2w),
    the four children added in the order ((a + b) + c) + d of `dtype`."""
    t = t.to(dtype)
    if mode == DOWN2:
        return R.nearest2(t, B, h, w) * 0.25
    assert mode == UP2
    s = t.reshape(B, 2 * h, 2 * w, -1)
    o = ((s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + s[:, 1::2, 0::2]) + s[:, 1::2, 1::2]
    return o.reshape(B * h * w, -1)


def resampled_dy(dy_at, mode, B, h, w):
    """The bf16 dy the backward uses for a dy given behind a resample: the adjoint summed in fp32
    (kernel order), rounded to bf16 once -- what the separate adjoint kernel would have stored."""
    return resample_adjoint(dy_at, mode, B, h, w, F32).to(BF16)


# ------------------------------------------------------------------ GroupNorm backward
def gn_bwd(x, B, HW, gamma, beta, mean, rstd, dy, film=None, use_silu=False, dsilu=None, prev=None,
           resid=None, resid_adj=None, dtype=F64):
    """Backward from GIVEN statistics.  z = (xh gamma + beta)(1 + scale) + shift, xh = (x - mean) rstd;
    dz = dy silu'(z) (silu'(z) read from `dsilu` when given); dn = dz (1 + scale).
    Returns dict: dx [B*HW][C] (+ prev: accumulate, + resid), dgamma / dbeta per-image partials
    [B][C], dscale / dshift [B][C] (None without FiLM).
    resid_adj: the skip branch's gradient already passed through its resample adjoint; it is added
    AFTER dx (with prev / without) was rounded to bf16."""
    C = x.shape[1]
    G = mean.shape[1]
    m = _per_channel(mean.to(dtype), C)
    r = _per_channel(rstd.to(dtype), C)
    ga, be = gamma.to(dtype), beta.to(dtype)
    xh = (x.to(dtype).reshape(B, HW, C) - m) * r
    n = xh * ga + be
    s1, sh = film_parts(film, B, C, dtype)
    z = n * s1 + sh if film is not None else n
    d = dy.to(dtype).reshape(B, HW, C)
    if use_silu:
        dz = d * (dsilu.to(dtype).reshape(B, HW, C) if dsilu is not None else silu_grad(z))
    else:
        dz = d
    dn = dz * s1 if film is not None else dz
    out = {"dbeta": dn.sum(1), "dgamma": (dn * xh).sum(1), "dscale": None, "dshift": None}
    if film is not None:
        out["dscale"] = (dz * n).sum(1)
        out["dshift"] = dz.sum(1)
    dxh = dn * ga
    cnt = HW * (C // G)
    m1 = _bg(dxh, B, HW, G).sum(dim=(1, 3)) / cnt
    m2 = _bg(dxh * xh, B, HW, G).sum(dim=(1, 3)) / cnt
    dx = r * (dxh - _per_channel(m1, C) - xh * _per_channel(m2, C))
    dx = dx.reshape(B * HW, C)
    if prev is not None:
        dx = dx + prev.to(dtype)
    if resid is not None:
        dx = dx + resid.to(dtype)
    if resid_adj is not None:
        out["dx_pre"], out["resid_adj"] = dx, resid_adj.to(dtype)  # the two terms, for two_rounding_slack()
        dx = dx.to(BF16).to(dtype) + resid_adj.to(dtype)
    out["dx"] = dx
    # error scales of the sums (sum |terms|), for bounds stated as a multiple of 2^-24 sum |terms|
    out["abs_dbeta"] = dn.abs().sum(1)
    out["abs_dgamma"] = (dn * xh).abs().sum(1)
    if film is not None:
        out["abs_dscale"] = (dz * n).abs().sum(1)
        out["abs_dshift"] = dz.abs().sum(1)
    return out


def two_rounding_slack(pre64, floor_pre):
    """dx + resid adjoint rounds dx to bf16 BEFORE the add.  A kernel whose unrounded dx lies within
    floor_pre of the fp64 one may round it to any bf16 value the interval [pre - floor, pre + floor]
    rounds to; per element the width of that set (0 wherever the whole interval rounds alike, one
    bf16 ulp of dx next to a rounding boundary).  Added to the bound of the bf16 rule, so the floor
    itself stays the fp32-vs-fp64 distance of the unrounded terms instead of absorbing fp32's own
    rounding flips (one flip anywhere would otherwise widen the floor of every element)."""
    lo = (pre64 - floor_pre).to(BF16).double()
    hi = (pre64 + floor_pre).to(BF16).double()
    return hi - lo


# ------------------------------------------------------------------ LayerNorm
def ln_fwd(x, gamma, beta, eps, dtype=F64):
    """(y, mean [rows], rstd [rows]); centred (two-pass) variance."""
    v = x.to(dtype)
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    return (v - mean) * rstd * gamma.to(dtype) + beta.to(dtype), mean[:, 0], rstd[:, 0]


def ln_bwd(x, gamma, mean, rstd, dy, prev=None, resid=None, dtype=F64):
    """From given (mean, rstd): (dx (+ prev)(+ resid), dy xh per row, dy per row) -- the two last are
    the summands of d gamma / d beta, summed by the caller into whatever partial rows it wants."""
    v, d, ga = x.to(dtype), dy.to(dtype), gamma.to(dtype)
    xh = (v - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    g = d * ga
    s1 = g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    dx = rstd.to(dtype)[:, None] * (g - s1 - xh * s2)
    if prev is not None:
        dx = dx + prev.to(dtype)
    if resid is not None:
        dx = dx + resid.to(dtype)
    return dx, d * xh, d


def ln_block_of_rows(rows, C, parts=LN_PARTS):
    """Partial row (workgroup) that owns each row in the bf16 backward: row r -> (r // RPB) % parts."""
    return (torch.arange(rows) // ln_rpb(C)) % parts


def ln_block_of_rows_f32(rows, parts):
    """fp32 backward: workgroup p owns the contiguous rows [p per, (p + 1) per), per = ceil(rows / parts)."""
    per = (rows + parts - 1) // parts
    return torch.arange(rows) // per


def partial_rows(terms, owner, parts):
    """Sum the per-row summands [rows][C] into [parts][C] by owner (rows without owner stay 0)."""
    out = torch.zeros(parts, terms.shape[1], dtype=terms.dtype, device=terms.device)
    return out.index_add_(0, owner.to(terms.device), terms)
