"""Restatement of the fused ResBlock conv (csrc/resconv.hip, encdiff_resconv_fwd), written from
include/encdiff_hip.h's description of EncdiffResConvArgs and the formulas of GroupNorm / FiLM / SiLU /
AvgPool2d(2) / nearest x2 / Conv2d(3, padding 1); no kernel code is imported.
tests/test_gpu_resconv_paths.py compares the HIP kernel with it per element;
tests/test_resconv_restate.py checks it on the CPU against torch.nn.functional in fp64.

Three parts:
  * RcPlan: a Python copy of rc_plan's arithmetic (the support domain, the tiling heuristic, the LDS
    layout) and of the path facts the kernel derives from it, so that every GPU case asserts the path
    it means to reach and the whole accepted domain can be checked for invariants on the CPU;
  * the reference: GN (+FiLM) (+SiLU) -> bf16 -> resample -> conv3x3 + bias + skip, dtype-generic
    (fp64: the reference; fp32: the evaluation whose distance from fp64 sets the additive floors);
  * the two-valued input builder of the exact cases and the case tables both test files import.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import elementwise_restate as R
import norm_restate as N

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NONE, DOWN2, UP2 = 0, 1, 2  # EncdiffResample (checked against _lib on the GPU)
OK, ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -3

# ------------------------------------------------------------------ plan (a copy of rc_plan's)
RC_THREADS = 512
RC_NW = RC_THREADS // 64
RC_PAD = 8
RC_LDS_MAX = 160 * 1024
RC_CE = 8


def _up16(n):
    return (n + 15) & ~15


class RcPlan:
    """What encdiff_resconv_fwd does with these arguments: rc (OK or the refusal's code) and, when
    planned, rc_plan's fields (ho, hwo, ipw, mc, wk, nchunk, ngroup, nsr, ncr, kl, lds, grid) and the
    path facts the kernel derives from them.  film: a FiLM pointer is given (film_addr its address
    modulo 16); resid: a residual pointer is given.  divisor_fix=False evaluates the heuristic as it
    was before the largest-divisor rule (kept to state the defect it had)."""

    def __init__(self, batch, h, cin, cout, resample=NONE, groups=32, film=False, ld_film=0, film_addr=0, cskip=0,
                 resid=False, resid_resample=NONE, tile_m=0, tile_n=0, skip_stages=0, ld_x=None, ld_w=None,
                 ld_y=None, ld_xskip=None, ld_wskip=None, divisor_fix=True):
        self.rc = self._plan(batch, h, cin, cout, resample, groups, film, ld_film, film_addr, cskip, resid,
                             resid_resample, tile_m, tile_n, skip_stages, cin if ld_x is None else ld_x,
                             9 * cin if ld_w is None else ld_w, cout if ld_y is None else ld_y,
                             cskip if ld_xskip is None else ld_xskip, cskip if ld_wskip is None else ld_wskip,
                             divisor_fix)
        self.ok = self.rc == OK

    def _plan(self, batch, h, cin, cout, resample, groups, film, ld_film, film_addr, cskip, resid, resid_resample,
              tile_m, tile_n, skip_stages, ld_x, ld_w, ld_y, ld_xskip, ld_wskip, divisor_fix):
        if batch <= 0 or h <= 0 or cin <= 0 or cin % 32 or cout % 16 or groups <= 0 or cin % groups:
            return ERR_SHAPE
        if ld_x % 8 or ld_w % 8 or ld_x < cin or ld_w < 9 * cin or ld_y < cout:
            return ERR_SHAPE
        if cin > 512 or groups > 64:
            return ERR_UNSUPPORTED
        if film and (film_addr % 16 or ld_film % 4):
            return ERR_UNSUPPORTED
        if not (0 <= resample <= 2 and 0 <= resid_resample <= 2):
            return ERR_ARG
        if resample == DOWN2 and h % 2:
            return ERR_SHAPE
        if cskip and (cskip % 32 or ld_xskip % 8 or ld_wskip % 8 or resid):
            return ERR_ARG
        self.ho = ho = 2 * h if resample == UP2 else h // 2 if resample == DOWN2 else h
        self.hwo = hwo = ho * ho
        if resid_resample == UP2 and ho % 2:
            return ERR_SHAPE
        if (hwo < 16 and 16 % hwo) or (hwo >= 16 and hwo % 16):
            return ERR_UNSUPPORTED
        self.ipw = ipw = 1 if hwo >= 16 else 16 // hwo
        if batch % ipw:
            return ERR_UNSUPPORTED
        self.nv = nv = cin // 8
        self.np = np_ = RC_THREADS // nv
        self.pow2 = nv & (nv - 1) == 0
        if np_ < ipw or ipw * cin > RC_CE * RC_THREADS:
            return ERR_UNSUPPORTED
        if not self.pow2 and ipw != 1:
            return ERR_UNSUPPORTED
        self.tn = tn = tile_n if tile_n else 1
        if tn not in (1, 2) or cout % (16 * tn):
            return ERR_ARG
        self.mtg = mtg = ipw * hwo // 16
        self.nslice = nslice = cout // (16 * tn)
        self.ngroup = ngroup = batch // ipw
        if tile_m:
            if tile_m not in (1, 2, 4) or mtg % tile_m:
                return ERR_ARG
            mc = tile_m
        else:
            if divisor_fix:  # the largest of 4, 2, 1 that divides mtg (halving keeps it a divisor)
                mc = 4 if mtg % 4 == 0 else 2 if mtg % 2 == 0 else 1
            else:
                mc = 4 if mtg >= 4 else 2 if mtg >= 2 else 1
            while mc > 1 and ngroup * (mtg // mc) * nslice < 256:
                mc >>= 1
        self.mc, self.wk = mc, RC_NW // mc
        self.nchunk = nchunk = mtg // mc
        self.ldx = ldx = cin + RC_PAD
        self.nsr = self.ncr = 0
        self.windows = []  # per chunk (cy0, cy1, sy0, sy1)
        for c in range(nchunk):
            cy0, cy1 = 0, ho - 1
            if ipw == 1:
                r0 = c * mc * 16
                r1 = r0 + mc * 16 - 1
                cy0, cy1 = max(r0 // ho - 1, 0), min(r1 // ho + 1, ho - 1)
            sy0 = cy0 >> 1 if resample == UP2 else 2 * cy0 if resample == DOWN2 else cy0
            sy1 = cy1 >> 1 if resample == UP2 else 2 * cy1 + 1 if resample == DOWN2 else cy1
            self.windows.append((cy0, cy1, sy0, sy1))
            self.nsr = max(self.nsr, sy1 - sy0 + 1)
            self.ncr = max(self.ncr, cy1 - cy0 + 1)
        off = _up16(ipw * self.nsr * h * ldx * 2)
        if resample == DOWN2:
            off += _up16(ipw * self.ncr * ho * ldx * 2)
        red_f = 2 * 16 * 64 if self.pow2 else 2 * RC_NW * cin
        kred_f = (self.wk - 1) * mc * 2 * tn * 256
        off += _up16(4 * max(red_f, kred_f))
        off += _up16(0 if self.pow2 else 8 * ipw * cin)
        off += _up16(8 * ipw * groups)
        off += _up16(8 * ipw * cin if film else 0)
        off += _up16(2 * cin)
        off += _up16((mc + tn) * (cskip // 32) * 1024)
        self.KS = KS = 9 * cin // 32
        room = (RC_LDS_MAX - off) // (1024 * tn)
        self.kl = 0 if room < 0 else (room & ~1 if room < KS else KS)
        if skip_stages & 64:
            self.kl = 0
        self.lds = off + self.kl * tn * 1024
        if self.lds > RC_LDS_MAX:
            return ERR_UNSUPPORTED
        self.grid = nslice * ngroup * nchunk
        # ---- path facts of the kernel
        self.xcd_remap = self.grid % 8 == 0
        self.cpg = cpg = cin // groups
        self.lpi = lpi = np_ // ipw                       # pixel lanes per image
        self.idle = RC_THREADS - lpi * ipw * nv          # threads without a pixel lane
        self.span = min(64, lpi * nv) if self.pow2 else None    # lanes of one image inside a wave
        self.nr = (lpi * nv // 64 if lpi * nv >= 64 else 1) if self.pow2 else None  # partial rows per image
        self.nslot = (groups if cpg <= 8 else nv) if self.pow2 else None
        self.streamed = self.kl < KS
        self.spt = cin // 32                              # k-steps per tap
        per = ((KS + self.wk - 1) // self.wk + 1) & ~1
        self.kranges = [(min(KS, i * per), min(KS, min(KS, i * per) + per)) for i in range(self.wk)]
        self.empty_waves = sum(1 for a, b in self.kranges if a == b)
        self.midtap_starts = sum(1 for a, b in self.kranges if a < b and a % self.spt)
        return OK


# ------------------------------------------------------------------ reference
def bf(t):
    """one round-to-nearest-even to bf16, back in the dtype it came in"""
    return t.to(BF16).to(t.dtype)


def film_rows(film, B):
    """A film of exactly 2 cin columns and one row is the ld_film = 0 form: ONE row for every image;
    otherwise [B][2 cin + 32] (film_ld)."""
    if film is None:
        return None
    return film.expand(B, -1) if film.shape[0] == 1 else film


def film_ld(film, cin):
    return 0 if film is None or film.shape[1] == 2 * cin else film.shape[1]


def pre_activation(x, B, h, groups, eps, gamma, beta, film=None, silu=True, dtype=F64):
    """act(GN(x)(1 + scale) + shift), unrounded, rows [B h h][cin]: one-pass statistics and the
    mul / add form of the bf16 GroupNorm kernels (norm_restate)."""
    mean, rstd = N.gn_stats_onepass(x, B, h * h, groups, eps, dtype)
    return N.gn_apply(x, B, h * h, gamma, beta, mean, rstd, film=film_rows(film, B), use_silu=silu, dtype=dtype)[0]


def pool_kernel_order(a, B, ho):
    """rows of (B, 2 ho, 2 ho) -> rows of (B, ho, ho), ((a + b) + c + d) / 4 in a's dtype"""
    s = a.reshape(B, 2 * ho, 2 * ho, -1)
    o = (((s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + s[:, 1::2, 0::2]) + s[:, 1::2, 1::2]) * 0.25
    return o.reshape(B * ho * ho, -1)


def resampled(a, B, h, mode):
    """The conv's input rows from the rounded activation: DOWN2 pooled and rounded to bf16 again, UP2
    nearest.  Returns (rows, ho)."""
    if mode == DOWN2:
        return bf(pool_kernel_order(a, B, h // 2)), h // 2
    if mode == UP2:
        return R.nearest2(a, B, 2 * h, 2 * h), 2 * h
    return a, h


def conv3x3_rows(a, B, ho, w):
    """rows [B ho ho][cin] x packed weights [cout][9 cin] (tap ky * 3 + kx major, channels last):
    zero padding at the conv resolution, one matmul per tap."""
    cin = a.shape[1]
    p = F.pad(a.reshape(B, ho, ho, cin), (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B * ho * ho, w.shape[0], dtype=a.dtype, device=a.device)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            y += p[:, ky:ky + ho, kx:kx + ho].reshape(-1, cin) @ w[:, t * cin:(t + 1) * cin].to(a.dtype).t()
    return y


def skip_term(B, ho, dtype, resid=None, resid_resample=NONE, xskip=None, wskip=None, bskip=None):
    """(the rounded term added to the conv, its unrounded value or None when nothing is rounded)"""
    if xskip is not None:
        s = xskip.to(dtype) @ wskip.to(dtype).t()
        if bskip is not None:
            s = s + bskip.to(dtype)
        return bf(s), s
    if resid is None:
        return None, None
    r = resid.to(dtype)
    if resid_resample == DOWN2:
        s = pool_kernel_order(r, B, ho)
        return bf(s), s
    if resid_resample == UP2:
        return R.nearest2(r, B, ho, ho), None
    return r, None


def resconv_ref(x, B, h, w, gamma, beta, eps, groups=32, film=None, silu=True, bias=None, resample=NONE, resid=None,
                resid_resample=NONE, xskip=None, wskip=None, bskip=None, dtype=F64, act=None):
    """The whole op.  Returns dict: pre (unrounded activation at h), a (the conv's bf16 input rows at
    ho), conv (unrounded conv + bias), skip / skip_pre, y (unrounded sum), out (its one RNE to bf16).
    act: use these conv-input rows instead of deriving them (stage-local checks)."""
    o = {}
    if act is None:
        o["pre"] = pre_activation(x, B, h, groups, eps, gamma, beta, film, silu, dtype)
        a, ho = resampled(bf(o["pre"]), B, h, resample)
    else:
        a, ho = act.to(dtype), (2 * h if resample == UP2 else h // 2 if resample == DOWN2 else h)
    o["a"], o["ho"] = a, ho
    y = conv3x3_rows(a, B, ho, w)
    if bias is not None:
        y = y + bias.to(dtype)
    o["conv"] = y
    o["skip"], o["skip_pre"] = skip_term(B, ho, dtype, resid, resid_resample, xskip, wskip, bskip)
    if o["skip"] is not None:
        y = y + o["skip"]
    o["y"] = y
    o["out"] = y.to(BF16)
    return o


# ------------------------------------------------------------------ bf16 rounding boundaries
def bf16_neighbours(r):
    """(next bf16 below, next above) of the bf16 tensor r, as fp64 (finite, non-zero r)"""
    b = r.view(torch.int16).to(torch.int32)
    mag = b & 0x7FFF
    up = (((mag + 1) | (b & 0x8000)) & 0xFFFF)
    dn = (((mag - 1) | (b & 0x8000)) & 0xFFFF)
    f = lambda v: (v - ((v & 0x8000) << 1)).to(torch.int16).view(BF16).double()  # noqa: E731
    away, toward = f(up), f(dn)   # larger / smaller magnitude
    return torch.minimum(away, toward), torch.maximum(away, toward)


def boundary_distance(v):
    """Distance of the fp64 values v (non-zero) to the nearest point where round-to-nearest-even to
    bf16 changes its result: the midpoints between bf16(v) and its two neighbours."""
    r = v.to(BF16)
    lo, hi = bf16_neighbours(r)
    rd = r.double()
    return torch.minimum(v - (lo + rd) / 2, (rd + hi) / 2 - v)


def bf16_ulp(v):
    """2^(floor(log2 |v|) - 7) of non-zero fp64 v"""
    return torch.exp2(torch.floor(torch.log2(v.abs())) - 7)


def quantum(a):
    """The largest power of two that divides every non-zero element of the bf16-valued tensor a
    (1.0 when all are zero): bf16 m 2^e with an 8-bit m has the unit 2^e 2^(trailing zeros of m)."""
    b = a.to(BF16).reshape(-1).view(torch.int16).to(torch.int32) & 0x7FFF
    b = b[b != 0]
    if b.numel() == 0:
        return 1.0
    e = (b >> 7)
    assert int(e.min()) > 0, "subnormal activation"
    m = (b & 0x7F) | 0x80
    tz = torch.zeros_like(m)
    for k in range(1, 8):
        tz = torch.where(m % (1 << k) == 0, torch.full_like(m, k), tz)
    return 2.0 ** int((e - 127 - 7 + tz).min())


# ------------------------------------------------------------------ the exact cases' inputs
# Lattice of the affine / FiLM parameters (all exact in fp32, every product of them too).
GAMMAS = (0.5, 1.0, 2.0)
BETAS = SHIFTS = (0.0, 0.5, -0.5, 1.0, -1.0)
SCALES = (-0.5, 0.0, 0.5, 1.0)
MARGIN_ULP = 2.0 ** -6   # required distance to a rounding boundary, in bf16 ulps of the value


def rstd_two_valued(eps):
    return 1.0 / math.sqrt(1.0 + eps)


# fp32 evaluation error of the kernel's activation on two-valued x (mean exactly 0, sum x^2 = n):
#   var   = n * fl(1 / n)              two roundings: (1 + d)^2, |d| <= 2^-24
#   var + eps                          one rounding
#   rstd  = rsqrtf(var + eps)          v_rsq_f32, 1 ulp = 2^-23; the argument's 3 * 2^-24 enters halved
#   mul   = rstd gamma (1 + scale)     gamma a power of two: exact; (1 + scale) = 3/2 rounds once
#   add   = beta (1 + scale) + shift   lattice values: exact
#   z     = +-mul + add                one rounding of z (fma or mul + add: +-1 * mul is exact)
RSTD_REL = 1.5 * 2.0 ** -24 + 2.0 ** -23
#   silu_f(z) = z * rcp(1 + __expf(-z)): e = exp(-z) carries st_restate.exp_rel_of(|z|) = 2^-23 (2 + |z|)
#   relative; 1 + e keeps at most that (e / (1 + e) < 1) plus its own rounding 2^-24; v_rcp_f32 1 ulp
#   2^-23; the product one rounding 2^-24.  An error dz of z moves silu by at most 1.1 |dz|
#   (max |silu'| = 1.0998).
SILU_REL_BASE = 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -24


def z_err(mul, z):
    """|kernel fp32 z - true z| bound: mul's relative error on |mul|, one rounding on |z|"""
    return mul.abs() * (RSTD_REL + 2.0 ** -24) + z.abs() * 2.0 ** -24


def act_slack(mul, z, silu):
    """|kernel fp32 activation - true activation| bound for true pre-activation z = +-mul + add"""
    ez = z_err(mul, z)
    if not silu:
        return ez
    return 1.1 * ez + R.silu(z).abs() * (2.0 ** -23 * (2 + z.abs()) + SILU_REL_BASE)


def lattice_table(eps, silu, zrange=None):
    """ok[gamma][beta][scale][shift]: for BOTH x = +1 and x = -1 the true activation is at least
    max(MARGIN_ULP bf16 ulps, the derived fp32 slack) away from every bf16 rounding boundary (and,
    zrange = (lo, hi): lo <= z <= hi, which bounds the activations' dynamic range for condition (c)).
    Also returns the number of passing (combination, sign) pairs and the smallest distance / slack
    ratio among them."""
    g = torch.tensor(GAMMAS, dtype=F64).view(-1, 1, 1, 1, 1)
    b = torch.tensor(BETAS, dtype=F64).view(1, -1, 1, 1, 1)
    sc = torch.tensor(SCALES, dtype=F64).view(1, 1, -1, 1, 1)
    sh = torch.tensor(SHIFTS, dtype=F64).view(1, 1, 1, -1, 1)
    sign = torch.tensor([1.0, -1.0], dtype=F64).view(1, 1, 1, 1, 2)
    mul = rstd_two_valued(eps) * g * (1 + sc) * torch.ones_like(b * sh * sign)
    z = sign * mul + b * (1 + sc) + sh
    v = R.silu(z) if silu else z
    dist = boundary_distance(v)
    slack = act_slack(mul, z, silu)
    ok = (dist >= MARGIN_ULP * bf16_ulp(v)) & (dist >= slack)
    if zrange is not None:
        ok &= (z >= zrange[0]) & (z <= zrange[1])
    ratio = (dist / slack)[ok].min().item() if ok.any() else float("inf")
    return ok.all(dim=-1), int(ok.sum()), ratio


def two_valued_x(g, B, hw, cin, groups):
    """x in {+1, -1}, balanced inside every (image, group): mean exactly 0, E[x^2] exactly 1 and
    every partial sum an integer in any order."""
    cpg = cin // groups
    n = hw * cpg
    assert n % 2 == 0, "hw * cpg must be even"
    base = torch.cat([torch.ones(n // 2), -torch.ones(n // 2)])
    perm = torch.rand(B * groups, n, generator=g).argsort(dim=1)
    v = base[perm].reshape(B, groups, hw, cpg)            # [B][G][hw][cpg]
    return v.permute(0, 2, 1, 3).reshape(B * hw, cin).to(BF16)


def draw_affine(g, B, cin, eps, silu, film, zrange=None):
    """gamma, beta [cin] and film ([B][2 cin], [1][2 cin] for film == 'one', None) from the lattice,
    only combinations lattice_table() passes: a failing draw is drawn again, never masked."""
    ok, _, _ = lattice_table(eps, silu, zrange)
    i_sc0, i_sh0 = SCALES.index(0.0), SHIFTS.index(0.0)
    rows = {None: 0, "one": 1, "rows": B}[film]
    if not rows:
        gb_ok = ok[:, :, i_sc0, i_sh0]
    else:
        gb_ok = ok.flatten(2).any(dim=2)
    gb = gb_ok.nonzero()
    assert len(gb), "no lattice combination passes"
    pick = gb[torch.randint(len(gb), (cin,), generator=g)]
    gamma = torch.tensor(GAMMAS)[pick[:, 0]]
    beta = torch.tensor(BETAS)[pick[:, 1]]
    if not rows:
        return gamma, beta, None
    flat = ok.flatten(2)[pick[:, 0], pick[:, 1]].double()             # [cin][scale x shift] 0 / 1
    idx = torch.multinomial(flat, rows, replacement=True, generator=g).t()  # [rows][cin]
    scale = torch.tensor(SCALES)[idx // len(SHIFTS)]
    shift = torch.tensor(SHIFTS)[idx % len(SHIFTS)]
    film_t = torch.cat([scale, shift], dim=1)
    if film == "rows":  # 32 columns behind scale | shift that must not be read
        film_t = torch.cat([film_t, torch.full((rows, 32), float("nan"))], dim=1)
    return gamma, beta, film_t


def small_ints(g, *shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# One exact case.  film: None / 'rows' (ld_film = 2 cin + 32) / 'one' (ld_film = 0); skip: None,
# ('conv', cskip, with_bskip) or ('resid', resid_resample); ss: skip_stages; want: the plan facts the
# case is there for (asserted before the launch).
Case = namedtuple("Case", "id B h cin cout rs groups silu film bias skip tm tn ss eps want")


def case(id, B, h, cin, cout, rs=NONE, groups=32, silu=True, film="rows", bias=True, skip=None, tm=0, tn=0, ss=0,
         eps=1e-5, **want):
    return Case(id, B, h, cin, cout, rs, groups, silu, film, bias, skip, tm, tn, ss, eps, want)


def plan_of(c, **kw):
    sk = c.skip or (None,)
    return RcPlan(c.B, c.h, c.cin, c.cout, resample=c.rs, groups=c.groups, film=c.film is not None,
                  ld_film={None: 0, "one": 0, "rows": 2 * c.cin + 32}[c.film], cskip=sk[1] if sk[0] == "conv" else 0,
                  resid=sk[0] == "resid", resid_resample=sk[1] if sk[0] == "resid" else NONE, tile_m=c.tm,
                  tile_n=c.tn, skip_stages=c.ss, **kw)


def expect_plan(p, want):
    assert p.ok, f"refused ({p.rc})"
    for k, v in want.items():
        got = getattr(p, k)
        assert got == v, f"plan changed: {k} = {got}, this case needs {v}"


ZR_SILU = (-2.5, 7.0)  # keeps silu's values within 2^-3 .. 2^3 so that condition (c) holds up to cin = 512

EXACT_CASES = [
    # ipw = 1, several chunks with halo rows at their borders; mc forced and heuristic; tile_n 1 / 2
    case("h8-c32-m1", 2, 8, 32, 32, tm=1, skip=("resid", NONE), ipw=1, mc=1, wk=8, nchunk=4, KS=9, empty_waves=3),
    case("h8-c32-m2n2", 2, 8, 32, 32, tm=2, tn=2, film="one", ipw=1, mc=2, wk=4, nchunk=2, nslice=1),
    case("h8-c32-m4", 1, 8, 32, 48, tm=4, silu=False, ipw=1, mc=4, wk=2, nchunk=1, xcd_remap=False),
    case("h8-c64-heur", 2, 8, 64, 32, skip=("conv", 32, True), ipw=1, mc=1, nchunk=4, xcd_remap=True),
    case("h16-c64-m4", 1, 16, 64, 16, tm=4, film=None, ipw=1, mc=4, nchunk=4, nsr=6),
    case("h16-c32-m2", 1, 16, 32, 32, tm=2, tn=2, bias=False, ipw=1, mc=2, nchunk=8, nsr=4),
    case("h16-c64-heur", 2, 16, 64, 32, skip=("resid", DOWN2), ipw=1, mc=1, nchunk=16, nsr=3),
    # ipw = 4: neighbours must not leak across the four images of a tile
    case("h2-c64", 8, 2, 64, 32, skip=("resid", UP2), ipw=4, mc=1, wk=8, ngroup=2),
    case("h4-down", 4, 4, 64, 32, rs=DOWN2, skip=("conv", 64, False), ipw=4, ho=2, ncr=2, nsr=4),
    case("h1-up", 4, 1, 64, 32, rs=UP2, film="one", skip=("resid", NONE), ipw=4, ho=2, nsr=1),
    # ipw = 16 (ho = 1): every tap but the centre reads the zero row
    case("h1-c64-b16", 16, 1, 64, 32, ipw=16, ho=1, lpi=4, ngroup=1),
    case("h1-c256-b32", 32, 1, 256, 16, silu=False, ipw=16, ho=1, lpi=1, ngroup=2, nr=1),
    case("h2-down-c64-b16", 16, 2, 64, 16, rs=DOWN2, skip=("resid", DOWN2), ipw=16, ho=1),
    case("h2-down-c256-b16", 16, 2, 256, 32, rs=DOWN2, film=None, skip=("conv", 192, True), ipw=16, ho=1, lpi=1),
    # widths that are not powers of two; mtg = 9 / 25: the heuristic must keep a divisor
    case("h12-b8-co256", 8, 12, 32, 256, skip=("resid", NONE), ipw=1, mtg=9, mc=1, nchunk=9, grid=1152),
    case("h12-b1", 1, 12, 32, 16, film=None, ipw=1, mtg=9, mc=1, nchunk=9, xcd_remap=False),
    case("h6-up-b8-co256", 8, 6, 32, 256, rs=UP2, skip=("resid", UP2), ipw=1, ho=12, mtg=9, mc=1),
    case("h24-down-b8-co256", 8, 24, 32, 256, rs=DOWN2, film="one", ipw=1, ho=12, mtg=9, mc=1, nchunk=9),
    case("h20-b4-co256", 4, 20, 32, 256, bias=False, ipw=1, mtg=25, mc=1, nchunk=25),
    # k-split ranges that start inside a tap (spt = 3), the non-power-of-two statistics path
    case("h8-c96-m1", 1, 8, 96, 32, tm=1, skip=("conv", 64, True), pow2=False, wk=8, midtap_starts=4, idle=8),
    case("h4-c96-heur", 2, 4, 96, 16, silu=False, skip=("resid", NONE), pow2=False, wk=8, mc=1),
    case("h8-c96-m4", 1, 8, 96, 16, tm=4, film=None, pow2=False, wk=2, midtap_starts=1),
    # kl < KS reached naturally (B streamed past the LDS budget), kl = KS beside it
    case("h8-c384-n2", 1, 8, 384, 32, tn=2, skip=("conv", 192, True), streamed=True, KS=108, pow2=False),
    case("h8-c384-m4", 1, 8, 384, 16, tm=4, film="one", streamed=True, mc=4),
    case("h2-c512", 4, 2, 512, 32, skip=("conv", 32, False), ipw=4, streamed=True, KS=144, cpg=16, nslot=64),
    case("h8-c256-m1", 1, 8, 256, 16, tm=1, skip=("resid", NONE), streamed=False, kl=72),
    # kl = 0: everything streamed (skip_stages = 64 keeps results correct)
    case("h8-c64-kl0", 1, 8, 64, 32, ss=64, tn=2, skip=("resid", NONE), kl=0, streamed=True),
    case("h2-c256-kl0", 4, 2, 256, 16, ss=64, silu=False, kl=0, streamed=True, ipw=4),
    # groups other than 32
    case("h4-c64-g8", 2, 4, 64, 16, groups=8, cpg=8, nslot=8),
    case("h4-c128-g8", 2, 4, 128, 16, groups=8, cpg=16, nslot=16, skip=("resid", UP2)),
    case("h4-c64-g64", 2, 4, 64, 16, groups=64, cpg=1, nslot=64, film=None, silu=False),
    # the shipped shapes (h 2 / 4 / 8 / 16, cin 64 .. 512): bitwise what they were
    case("ship-16x16-64", 8, 16, 64, 64, skip=("resid", NONE), mc=2, nchunk=8, grid=256),
    case("ship-16x16-192", 8, 16, 192, 64, skip=("conv", 128, True), mc=2, pow2=False),
    case("ship-8x8-384", 8, 8, 384, 128, skip=("conv", 256, True), mc=1, wk=8),
    case("ship-8x8-up", 8, 8, 128, 128, rs=UP2, film=None, skip=("resid", UP2), ho=16, mc=4),
    case("ship-4x4-down", 8, 4, 256, 256, rs=DOWN2, film=None, ipw=4, ho=2),
    case("ship-2x2-512", 8, 2, 512, 256, skip=("conv", 256, True), ipw=4, streamed=True),
]


def exact_inputs(c, seed=0):
    """The exact case's tensors (CPU): x two-valued, affine / FiLM from the lattice, integer weights,
    bias, residual and skip operands."""
    g = torch.Generator().manual_seed(1000 + seed)
    ho = 2 * c.h if c.rs == UP2 else c.h // 2 if c.rs == DOWN2 else c.h
    t = {"x": two_valued_x(g, c.B, c.h * c.h, c.cin, c.groups)}
    t["gamma"], t["beta"], t["film"] = draw_affine(g, c.B, c.cin, c.eps, c.silu, c.film, ZR_SILU if c.silu else None)
    t["w"] = small_ints(g, c.cout, 9 * c.cin).to(BF16)
    t["bias"] = small_ints(g, c.cout, lo=-2, hi=2) if c.bias else None
    t["resid"] = t["xskip"] = t["wskip"] = t["bskip"] = None
    t["resid_resample"] = NONE
    if c.skip and c.skip[0] == "conv":
        t["xskip"] = small_ints(g, c.B * ho * ho, c.skip[1], lo=-2, hi=2).to(BF16)
        t["wskip"] = small_ints(g, c.cout, c.skip[1]).to(BF16)
        t["bskip"] = small_ints(g, c.cout, lo=-2, hi=2) if c.skip[2] else None
    elif c.skip:
        hr = ho // 2 if c.skip[1] == UP2 else 2 * ho if c.skip[1] == DOWN2 else ho
        t["resid"] = small_ints(g, c.B * hr * hr, c.cout, lo=-3, hi=3).to(BF16)
        t["resid_resample"] = c.skip[1]
    return t


def exact_reference(c, t):
    return resconv_ref(t["x"], c.B, c.h, t["w"], t["gamma"], t["beta"], c.eps, groups=c.groups, film=t["film"],
                       silu=c.silu, bias=t["bias"], resample=c.rs, resid=t["resid"],
                       resid_resample=t["resid_resample"], xskip=t["xskip"], wskip=t["wskip"], bskip=t["bskip"])


def exact_conditions(c, t, ref=None):
    """The three conditions under which the kernel's fp32 arithmetic must reproduce the fp64
    reference bit for bit.  Returns dict: margin (smallest distance of a true activation to a bf16
    rounding boundary, in units of the derived fp32 slack; must be >= 1), margin_ulp (the same in
    bf16 ulps; must be >= MARGIN_ULP), q (the quantum of the conv's input rows), bound (the largest
    sum |w| |a| / q + the epilogue's terms of any output; must be < 2^24), skip_bound."""
    ref = exact_reference(c, t) if ref is None else ref
    pre = ref["pre"]
    B, hw, cin = c.B, c.h * c.h, c.cin
    # (a) on the true pre-activation z and its mul (recovered from the parameters, not from x)
    s1 = 1.0
    if t["film"] is not None:
        s1 = (1 + film_rows(t["film"], B)[:, :cin].double()).reshape(B, 1, cin)
    mul = (rstd_two_valued(c.eps) * t["gamma"].double() * s1 * torch.ones(B, hw, cin, dtype=F64)).reshape(B * hw, cin)
    if c.silu:  # pre = silu(z): z from the parameters
        add = t["beta"].double() * s1
        if t["film"] is not None:
            add = add + film_rows(t["film"], B)[:, cin:2 * cin].double().reshape(B, 1, cin)
        z = t["x"].double() * mul + (add * torch.ones(B, hw, cin, dtype=F64)).reshape(B * hw, cin)
    else:
        z = pre
    assert (pre != 0).all()
    dist = boundary_distance(pre)
    out = {"margin": (dist / act_slack(mul, z, c.silu)).min().item(),
           "margin_ulp": (dist / bf16_ulp(pre)).min().item()}
    # (b), (c): everything the MFMA accumulates is an integer multiple of q and stays below 2^24 q
    a = ref["a"]
    out["q"] = q = quantum(a)
    assert torch.equal(torch.round(a / q), a / q)
    bound = conv3x3_rows(a.abs(), B, ref["ho"], t["w"].double().abs())
    if t["bias"] is not None:
        bound = bound + t["bias"].double().abs()
    if ref["skip"] is not None:
        bound = bound + ref["skip"].abs()
    out["bound"] = (bound / min(q, 1.0)).max().item()
    out["skip_bound"] = 0.0
    if t["xskip"] is not None:
        sb = t["xskip"].double().abs() @ t["wskip"].double().abs().t()
        if t["bskip"] is not None:
            sb = sb + t["bskip"].double().abs()
        out["skip_bound"] = sb.max().item()
    if c.rs == DOWN2:  # the pool's fp32 sum of four rounded activations is exact too
        a0 = bf(pre)
        q0 = quantum(a0)
        out["pool_bound"] = (4 * a0.abs().max() / q0).item()
    return out


def assert_exact_conditions(cond):
    assert cond["margin"] >= 1.0 and cond["margin_ulp"] >= MARGIN_ULP, cond
    assert cond["bound"] < 2 ** 24 and cond["skip_bound"] < 2 ** 24 and cond.get("pool_bound", 0) < 2 ** 24, cond


# ------------------------------------------------------------------ Gaussian cases (probe / contraction)
# Activation probe: (id, B, h, cin, groups, rs, want)
PROBE_CASES = [
    ("c32", 2, 4, 32, 32, NONE, dict(nv=4, pow2=True, cpg=1, ipw=1, span=64, nr=8)),
    ("c64", 2, 8, 64, 32, NONE, dict(nv=8, cpg=2, ipw=1, nr=8)),
    ("c128", 2, 4, 128, 32, NONE, dict(nv=16, cpg=4, nr=8)),
    ("c256", 1, 8, 256, 32, NONE, dict(nv=32, cpg=8, nslot=32)),
    ("c512", 1, 4, 512, 32, NONE, dict(nv=64, cpg=16, nslot=64, span=64)),
    ("c64-g8", 2, 4, 64, 8, NONE, dict(cpg=8, nslot=8)),
    ("c128-g8", 2, 4, 128, 8, NONE, dict(cpg=16, nslot=16)),
    ("c64-g64", 2, 4, 64, 64, NONE, dict(cpg=1, nslot=64)),
    ("c512-g64", 1, 4, 512, 64, NONE, dict(cpg=8, nslot=64)),
    ("ipw4-c64", 4, 2, 64, 32, NONE, dict(ipw=4, lpi=16, span=64, nr=2)),
    ("ipw4-c512", 4, 2, 512, 32, NONE, dict(ipw=4, lpi=2, nr=2)),
    ("ipw16-c64", 16, 1, 64, 32, NONE, dict(ipw=16, lpi=4, span=32, nr=1)),
    ("ipw16-c256", 16, 1, 256, 32, NONE, dict(ipw=16, lpi=1, span=32, nr=1)),
    ("ipw4-down", 4, 4, 128, 32, DOWN2, dict(ipw=4, ho=2)),
    ("ipw16-down", 16, 2, 64, 32, DOWN2, dict(ipw=16, ho=1)),
    ("down-h8", 2, 8, 64, 32, DOWN2, dict(ipw=1, ho=4)),
    ("up-h4", 2, 4, 64, 32, UP2, dict(ipw=1, ho=8)),
    ("up-h1", 4, 1, 64, 32, UP2, dict(ipw=4, ho=2)),
    ("c96", 2, 4, 96, 32, NONE, dict(pow2=False, nv=12, idle=8)),
    ("c160", 1, 8, 160, 32, NONE, dict(pow2=False, nv=20, idle=12)),
    ("c192", 1, 4, 192, 32, NONE, dict(pow2=False, nv=24, idle=8)),
    ("c320", 1, 4, 320, 32, NONE, dict(pow2=False, nv=40, idle=32)),
    ("c384", 1, 8, 384, 32, NONE, dict(pow2=False, nv=48, idle=32)),
    ("c448", 1, 4, 448, 32, NONE, dict(pow2=False, nv=56, idle=8)),
    ("c96-h12", 1, 12, 96, 32, NONE, dict(pow2=False, mtg=9, mc=1)),
]
# option sets of the probe: (film, silu, eps)
PROBE_OPTS = [("rows", True, 1e-5), (None, True, 1e-6), ("rows", False, 1e-6), (None, False, 1e-5)]

# Rounded contraction, one per path family: (id, B, h, cin, cout, rs, skip, tm, tn, want)
CONTRACT_CASES = [
    ("ipw1-c96", 2, 8, 96, 32, NONE, ("conv", 64, True), 0, 0, dict(ipw=1, pow2=False)),
    ("ipw1-m4-c64", 1, 16, 64, 32, NONE, ("resid", NONE), 4, 2, dict(ipw=1, mc=4, wk=2)),
    ("ipw4-c128", 4, 2, 128, 32, NONE, ("resid", UP2), 0, 0, dict(ipw=4, wk=8)),
    ("ipw16-c64", 16, 1, 64, 32, NONE, None, 0, 0, dict(ipw=16)),
    ("stream-c512", 4, 2, 512, 32, NONE, ("conv", 32, False), 0, 0, dict(streamed=True)),
    ("down-c64", 2, 8, 64, 32, DOWN2, ("resid", DOWN2), 0, 0, dict(ho=4)),
    ("up-c64-h6", 1, 6, 64, 32, UP2, None, 0, 0, dict(ho=12, mtg=9, mc=1)),
]

# Refusals, one per line of rc_plan: (id, RcPlan keyword arguments, the code)
REFUSALS = [
    ("cin%32", dict(batch=2, h=4, cin=48, cout=32, groups=16), ERR_SHAPE),
    ("cout%16", dict(batch=2, h=4, cin=64, cout=24), ERR_SHAPE),
    ("cin>512", dict(batch=2, h=4, cin=544, cout=32), ERR_UNSUPPORTED),
    ("groups>64", dict(batch=2, h=4, cin=128, cout=32, groups=128), ERR_UNSUPPORTED),
    ("cin%groups", dict(batch=2, h=4, cin=64, cout=32, groups=24), ERR_SHAPE),
    ("h3", dict(batch=2, h=3, cin=64, cout=32), ERR_UNSUPPORTED),
    ("h6", dict(batch=2, h=6, cin=64, cout=32), ERR_UNSUPPORTED),
    ("batch%ipw", dict(batch=6, h=2, cin=64, cout=32), ERR_UNSUPPORTED),
    ("nonpow2-ipw4", dict(batch=4, h=2, cin=96, cout=32), ERR_UNSUPPORTED),
    ("ipw*cin>4096", dict(batch=16, h=1, cin=512, cout=32), ERR_UNSUPPORTED),
    ("odd-h-down", dict(batch=2, h=5, cin=64, cout=32, resample=DOWN2), ERR_SHAPE),
    ("resid-up-odd-ho", dict(batch=16, h=1, cin=64, cout=32, resid=True, resid_resample=UP2), ERR_SHAPE),
    ("film-misaligned", dict(batch=2, h=4, cin=64, cout=32, film=True, ld_film=160, film_addr=4), ERR_UNSUPPORTED),
    ("ld_film%4", dict(batch=2, h=4, cin=64, cout=32, film=True, ld_film=162), ERR_UNSUPPORTED),
    ("cskip+resid", dict(batch=2, h=4, cin=64, cout=32, cskip=32, resid=True), ERR_ARG),
    ("cskip%32", dict(batch=2, h=4, cin=64, cout=32, cskip=48), ERR_ARG),
    ("tile_m-mtg", dict(batch=2, h=4, cin=64, cout=32, tile_m=2), ERR_ARG),
    ("tile_m-h12", dict(batch=2, h=12, cin=32, cout=32, tile_m=4), ERR_ARG),
    ("tile_n2-cout%32", dict(batch=2, h=4, cin=64, cout=48, tile_n=2), ERR_ARG),
    ("lds-h32-c512", dict(batch=1, h=32, cin=512, cout=32, resample=DOWN2), ERR_UNSUPPORTED),  # 6 staged rows
]
