"""Per-element and exact tests of the fused ResBlock conv (csrc/resconv.hip, encdiff_resconv_fwd) on
every path its plan can take, on the MI355X.  tests/test_gpu_resconv.py holds the UNet's nine shapes
to norm-level bounds; one unwritten row, a tap read across an image border or a lost k-split partial
of one wave does not move a norm, so here

  (a) exact cases, zero tolerance: x in {+1, -1} balanced inside every (image, group), so the
      statistics are exactly (0, (1 + eps)^-1/2) in any summation order; affine / FiLM parameters
      from a lattice of powers of two and halves, only combinations whose true activation stays clear
      of every bf16 rounding boundary by more than the fp32 evaluation can move it; integer weights,
      bias, residual and skip operands, with sum |w| |a| below 2^24 quanta.  Every fp32 sum is then
      exact in any order and the output must equal the fp64 reference's single round-to-nearest-even
      bit for bit (tests/resconv_restate.py; the conditions are checked on the CPU for the same case
      table by tests/test_resconv_restate.py);
  (b) an activation probe on Gaussian data: cout = cin and w = the identity on the centre tap make y
      bitwise the bf16 activation the kernel holds in LDS (after DOWN2 / UP2); compared per element
      with the fp64 GroupNorm restatement under the bf16 rule |out - ref| <= 2^-7 |ref| + floor,
      floor = 4 x the largest |fp32 evaluation - fp64| of the same one-pass restatement (DOWN2: +
      norm_restate.two_rounding_slack for the rounding before the pool);
  (c) one rounded contraction per path family, stage-local: Gaussian weights, the fp64 conv of the
      activation the probe observed for the same inputs, the bf16 rule with the floor measured the
      same way (+ two_rounding_slack where the skip term is rounded before it is added);
  (d) one refusal per line of rc_plan, with y untouched.
Every case asserts the plan it means to reach (resconv_restate.RcPlan) and that plan's lds / grid
against encdiff_resconv_query before it launches; y is a view with ld_y > cout inside a sentinel
buffer, pre-filled with NaN; operands are placed contiguous and as offset views with NaN around them
(ld % 8 == 0, 16-byte aligned bases: the kernel does not check pointer alignment); FiLM rows have 32
NaN columns behind scale | shift; every launch runs twice (once through ops.resconv_fwd, once
through the entry point directly) and must agree bitwise.

Kernel branch -> test
  rc_plan: mc heuristic keeps a divisor of mtg (12x12, 20x20: fixed here) ... test_exact[h12-*, h6-up-*, h24-down-*, h20-*]
  grid remap on (grid % 8 == 0) / off ................................... test_exact[h8-c64-heur / h8-c32-m4, h12-b1]
  ipw 1: chunks, halo rows at chunk borders, mc 1 / 2 / 4, tile_n 1 / 2 .. test_exact[h8-*, h16-*]
  ipw 4: four images per tile, no leak across them ........................ test_exact[h2-c64, h4-down, h1-up]
  ipw 16 (ho = 1): all taps but the centre read the zero row .............. test_exact[h1-*, h2-down-*]
  LDS-DMA of B / skip fragments / FiLM rows, ld_film 0 .................... test_exact (film 'rows' / 'one' / None)
  statistics, power-of-two nv: shuffles 4 / 8, permlane 16 / 32, nr rows,
    group slots (cpg <= 8) and vector slots (cpg 16) ...................... test_probe[c32 .. c512, *-g8, *-g64, ipw*]
  statistics, other nv: wave rows through LDS, idle threads ............... test_probe[c96 .. c448]
  one-pass variance at |mean| / std 1, 16, 64 ............................. test_probe_conditioning
  normalise: FiLM x SiLU, eps ............................................. test_probe (four option sets)
  DOWN2 pool into ps, ((a + b) + c + d) / 4 ............................... test_probe[*down*], test_exact[*down*]
  UP2 gather through >> 1 ................................................. test_probe[up-*], test_exact[h1-up, h6-up-*, ship-8x8-up]
  statistics independent of the plan ...................................... test_probe_same_under_every_tiling
  gather: padding taps (zr), tap and channel order ........................ test_exact (every case)
  k loop: B from LDS (kl = KS), streamed past kl, kl = 0 ................... test_exact[*c384*, h2-c512, *kl0]
  k-split 2 / 4 / 8 waves, empty ranges, ranges starting inside a tap ..... test_exact[h8-c32-m*, h8-c96-*]
  skip conv k loop (cskip 32 / 64 / 192 / 256), bskip NULL ................. test_exact[*conv*]
  residual prefetch NONE / UP2 / DOWN2; bias NULL; no skip ................ test_exact
  fp32 accumulation at non-integer magnitudes ............................. test_contraction
  every refusal of rc_plan ................................................ test_refusals

Measured on the MI355X (every case prints its own figures): 138 cases in 2.8 s, the slowest 0.3 s
(the first launch).  Exact: 74 cases, 0 differing elements; the largest sum |w| |a| + epilogue terms is
2^21.1 quanta; the smallest distance of a true activation to a rounding boundary is 0.0163 bf16 ulp
(required: 2^-6 = 0.0156) = 48 x the derived fp32 slack of that element (SiLU at |z| <= 7: the slack
is at most 1.1 |dz| + |silu| 2^-23 (2 + |z| + 2), about 1.3e-6 relative; over the whole lattice the
smallest distance / slack is 8.8).  Probe: largest floor 2.1e-4, largest |out - ref| 3.0e-2 (values
up to ~8: 2^-7 |ref| = 6e-2); conditioning at |mean| / std = 64: floor up to 4.0e-3, |out - ref| up to
1.6e-2.  Contraction: largest floor 4.1e-6, largest |out - ref| 1.5e-2.
On the commit before the heuristic's fix the h12 / h6-up / h24-down cases at B = 8, cout = 256 leave
rows 128..143 of every image NaN (mc = 4, two chunks for nine tiles); rows 0..127 are exact.
"""
import ctypes
import functools

import pytest
import torch

import elementwise_restate as R
import norm_restate as N
import resconv_restate as RR
from resconv_restate import DOWN2, NONE, UP2
from test_gpu_elementwise import Guard

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
    assert (lib.RESAMPLE_NONE, lib.RESAMPLE_DOWN2, lib.RESAMPLE_UP2) == (NONE, DOWN2, UP2)
    return ops


@pytest.fixture(scope="module")
def L():
    import encdiff_amd._lib as lib
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def placed(t, strided):
    """t on the device: contiguous, or an offset view (first column 8, row stride + 24) with NaN
    around it; None stays None."""
    if t is None:
        return None
    t = t.to(dev)
    if not strided:
        return t.contiguous()
    return Guard(t.shape[0], t.shape[1], t.dtype, strided=True, init=t, fill=NAN).view


def film_placed(film, cin):
    """'rows': [B][2 cin + 32] with NaN behind scale | shift; 'one': a single row, ld_film = 0"""
    if film is None:
        return None, 0
    return film.to(dev).float().contiguous(), RR.film_ld(film, cin)


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(O, L, plan, B, h, cin, cout, t, rs=NONE, groups=32, silu=True, eps=1e-5, tm=0, tn=0, ss=0, strided=False):
    """Query (lds / grid against the plan), launch twice into NaN-filled guarded outputs -- through
    ops.resconv_fwd (no skip_stages) and through the entry point -- and return the agreed output."""
    ho = plan.ho
    d = {k: placed(t.get(k), strided) for k in ("x", "w", "resid", "xskip", "wskip")}
    f = {k: None if t.get(k) is None else t[k].to(dev).float() for k in ("gamma", "beta", "bias", "bskip")}
    E, ld_film = film_placed(t.get("film"), cin)
    rr = t.get("resid_resample", NONE)
    outs = []
    for way in ("ops", "entry"):
        y = Guard(B * ho * ho, cout, BF16, strided=True, init=torch.full((B * ho * ho, cout), NAN, device=dev))
        a = L.ResConvArgs(batch=B, h=h, cin=cin, cout=cout, resample=rs, groups=groups, silu=int(silu), eps=eps,
                          x=_ptr(d["x"]), ld_x=d["x"].stride(0), gamma=_ptr(f["gamma"]), beta=_ptr(f["beta"]),
                          film=_ptr(E), ld_film=ld_film, w=_ptr(d["w"]), ld_w=d["w"].stride(0), bias=_ptr(f["bias"]),
                          y=_ptr(y.view), ld_y=y.view.stride(0), tile_m=tm, tile_n=tn, skip_stages=ss)
        if d["resid"] is not None:
            a.resid, a.ld_resid, a.resid_resample = _ptr(d["resid"]), d["resid"].stride(0), rr
        if d["xskip"] is not None:
            a.cskip, a.xskip, a.ld_xskip = d["xskip"].shape[1], _ptr(d["xskip"]), d["xskip"].stride(0)
            a.wskip, a.ld_wskip, a.bskip = _ptr(d["wskip"]), d["wskip"].stride(0), _ptr(f["bskip"])
        lds, grid = ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.lib.encdiff_resconv_query(ctypes.byref(a), ctypes.byref(lds), ctypes.byref(grid)) == 0
        assert (lds.value, grid.value) == (plan.lds, plan.grid), (lds.value, grid.value, plan.lds, plan.grid)
        if way == "ops" and ss == 0:
            old = O.RC_TILE_M, O.RC_TILE_N
            O.RC_TILE_M, O.RC_TILE_N = tm, tn
            try:
                assert O.resconv_fwd(d["x"], O.Geom(B, h, h), d["w"], y.view, f["gamma"], f["beta"], eps, silu=silu,
                                     film=E, ld_film=ld_film, bias=f["bias"], resample=rs, resid=d["resid"],
                                     resid_resample=rr, xskip=d["xskip"], wskip=d["wskip"], bskip=f["bskip"],
                                     groups=groups)
            finally:
                O.RC_TILE_M, O.RC_TILE_N = old
        else:
            L.check(L.lib.encdiff_resconv_fwd(ctypes.byref(a), _stream()), "encdiff_resconv_fwd")
        torch.cuda.synchronize()
        y.check()
        outs.append(y.view.clone())
    assert R.same_bits(outs[0], outs[1]), "two launches of the same arguments differ"
    return outs[0].cpu()


def unwritten(out, hwo):
    """'image-relative rows still NaN' for the failure message"""
    rows = out.float().isnan().any(dim=1).nonzero().flatten()
    return sorted({int(r) % hwo for r in rows})


# ====================================================================== (a) exact cases
@functools.lru_cache(maxsize=None)
def _exact(i):
    c = RR.EXACT_CASES[i]
    t = RR.exact_inputs(c)
    ref = RR.exact_reference(c, t)
    cond = RR.exact_conditions(c, t, ref)
    RR.assert_exact_conditions(cond)
    return t, ref, cond


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("i", range(len(RR.EXACT_CASES)), ids=[c.id for c in RR.EXACT_CASES])
def test_exact(O, L, i, strided):
    """The output equals the fp64 reference's one RNE to bf16 bit for bit (after + 0: the sign of a
    zero is not pinned).  An unwritten row (NaN), a tap read across an image or chunk border, a lost
    or doubled k-split partial, a wrong kl boundary, a pooled term or a residual pixel shows as a
    difference of at least one quantum."""
    c = RR.EXACT_CASES[i]
    plan = RR.plan_of(c)
    RR.expect_plan(plan, c.want)
    t, ref, cond = _exact(i)
    out = launch(O, L, plan, c.B, c.h, c.cin, c.cout, t, rs=c.rs, groups=c.groups, silu=c.silu, eps=c.eps, tm=c.tm,
                 tn=c.tn, ss=c.ss, strided=strided)
    want = ref["out"]
    bad = (R.bits(out + 0) != R.bits(want + 0)).sum().item()
    print(f"{c.id}: mc {plan.mc} wk {plan.wk} nchunk {plan.nchunk} kl {plan.kl}/{plan.KS} grid {plan.grid} lds {plan.lds}"
          f" q {cond['q']} bound 2^{torch.tensor(cond['bound']).log2().item():.1f} margin {cond['margin']:.1f} slacks"
          f" ({cond['margin_ulp']:.4f} ulp): {bad} of {out.numel()} elements differ")
    assert R.same_bits(out + 0, want + 0), (f"{bad} elements differ, max |out - ref| "
                                            f"{(out.double() - want.double()).abs().nan_to_num(1e30).max().item():.3g}, "
                                            f"unwritten rows of an image: {unwritten(out, plan.hwo)}")


# ====================================================================== (b) activation probe
@functools.lru_cache(maxsize=None)
def _identity_w(cin):
    w = torch.zeros(cin, 9 * cin)
    w[torch.arange(cin), 4 * cin + torch.arange(cin)] = 1.0
    return w.to(BF16)


def _gauss_inputs(seed, B, h, cin, film, x=None):
    g = torch.Generator().manual_seed(seed)
    t = {"x": ((torch.randn(B * h * h, cin, generator=g) * 2.0 + 0.5).to(BF16) if x is None else x),
         "gamma": 1 + 0.3 * torch.randn(cin, generator=g), "beta": 0.3 * torch.randn(cin, generator=g)}
    t["film"] = {None: None, "rows": 0.3 * torch.randn(B, 2 * cin + 32, generator=g),
                 "one": 0.3 * torch.randn(1, 2 * cin, generator=g)}[film]
    if film == "rows":
        t["film"][:, 2 * cin:] = NAN
    return t


def probe(O, L, B, h, cin, groups, rs, t, silu, eps, tm=0, tn=0, strided=False, want=None):
    plan = RR.RcPlan(B, h, cin, cin, resample=rs, groups=groups, film=t["film"] is not None,
                     ld_film=RR.film_ld(t["film"], cin), tile_m=tm, tile_n=tn)
    RR.expect_plan(plan, want or {})
    tt = dict(t, w=_identity_w(cin), bias=None)
    return launch(O, L, plan, B, h, cin, cin, tt, rs=rs, groups=groups, silu=silu, eps=eps, tm=tm, tn=tn,
                  strided=strided), plan


def check_probe(out, t, B, h, groups, rs, silu, eps, what):
    """bf16 rule on the observed activation; floor from the fp32 evaluation of the same restatement"""
    p64 = RR.pre_activation(t["x"], B, h, groups, eps, t["gamma"], t["beta"], t["film"], silu, F64)
    p32 = RR.pre_activation(t["x"], B, h, groups, eps, t["gamma"], t["beta"], t["film"], silu, F32)
    floor = R.floor_of(p32, p64)
    if rs == DOWN2:
        ref = RR.pool_kernel_order(RR.bf(p64), B, h // 2)
        slack = RR.pool_kernel_order(N.two_rounding_slack(p64, floor), B, h // 2)
    else:
        ref = R.nearest2(p64, B, 2 * h, 2 * h) if rs == UP2 else p64
        slack = torch.zeros_like(ref)
    err = (out.double() - ref).abs()
    ex = (err - (2.0 ** -7 * ref.abs() + floor + slack)).max().item()
    print(f"{what}: floor {floor:.3e} max|out-ref| {err.max().item():.3e} excess {ex:.3e}")
    assert ex <= 0, f"{what}: an element exceeds 2^-7 |ref| + {floor:.3e} by {ex:.3e}"


@pytest.mark.parametrize("id_,B,h,cin,groups,rs,want", RR.PROBE_CASES, ids=[p[0] for p in RR.PROBE_CASES])
def test_probe(O, L, id_, B, h, cin, groups, rs, want):
    """The four option sets (FiLM x SiLU, eps 1e-5 / 1e-6) on every statistics path; operands strided
    on the odd sets."""
    for k, (film, silu, eps) in enumerate(RR.PROBE_OPTS):
        t = _gauss_inputs(7 * cin + h + k, B, h, cin, film)
        out, _ = probe(O, L, B, h, cin, groups, rs, t, silu, eps, strided=bool(k % 2), want=want)
        check_probe(out, t, B, h, groups, rs, silu, eps, f"{id_} film {film} silu {silu} eps {eps}")


@pytest.mark.parametrize("ratio", [1, 16, 64])
@pytest.mark.parametrize("B,h,cin,pow2", [(2, 8, 64, True), (2, 4, 96, False), (4, 2, 128, True)])
def test_probe_conditioning(O, L, B, h, cin, pow2, ratio):
    """var = E[x^2] - mean^2 in one fp32 pass loses log2(ratio^2) bits: groups with |mean| / std = 1,
    16, 64 (alternating sign per group, as test_gpu_norm.test_gn_fwd_conditioning).  The floor is the
    fp32 evaluation of the same one-pass form, so the kernel's sums may be no worse than that."""
    off, sigma = (1.0, 1.0) if ratio == 1 else (1.9375, 1.9375 / ratio)
    g = torch.Generator().manual_seed(ratio + cin)
    sign = torch.where(torch.arange(32) % 2 == 0, 1.0, -1.0).repeat_interleave(cin // 32)
    x = (torch.randn(B * h * h, cin, generator=g) * sigma + off * sign).to(BF16)
    for k, (film, silu, eps) in enumerate(RR.PROBE_OPTS[:2]):
        t = _gauss_inputs(50 + k, B, h, cin, film, x=x)
        out, _ = probe(O, L, B, h, cin, 32, NONE, t, silu, eps, want=dict(pow2=pow2))
        check_probe(out, t, B, h, 32, NONE, silu, eps, f"ratio {ratio} cin {cin} h {h} film {film}")


@pytest.mark.parametrize("B,h,cin,rs,tiles", [
    (2, 8, 64, NONE, [(0, 0), (1, 1), (2, 2), (4, 1), (1, 2)]),
    (1, 16, 96, DOWN2, [(0, 0), (1, 2), (2, 1), (4, 2)]),
    (2, 4, 128, UP2, [(0, 0), (1, 2), (2, 1), (4, 1)])])
def test_probe_same_under_every_tiling(O, L, B, h, cin, rs, tiles):
    """The statistics and the normalisation do not depend on the plan: the probe's output is bitwise
    the same for every tile_m / tile_n."""
    t = _gauss_inputs(h + cin, B, h, cin, "rows")
    outs = [probe(O, L, B, h, cin, 32, rs, t, True, 1e-5, tm=tm, tn=tn)[0] for tm, tn in tiles]
    for o, tl in zip(outs[1:], tiles[1:]):
        assert R.same_bits(o, outs[0]), f"tiles {tl} change the activation"


# ====================================================================== (c) rounded contraction
@pytest.mark.parametrize("id_,B,h,cin,cout,rs,skip,tm,tn,want", RR.CONTRACT_CASES, ids=[c[0] for c in RR.CONTRACT_CASES])
def test_contraction(O, L, id_, B, h, cin, cout, rs, skip, tm, tn, want):
    """Gaussian weights on Gaussian data, checked from the activation the probe observed for the same
    inputs: out against conv3x3_fp64(observed) + bias + skip under the bf16 rule, floor = 4 x the
    largest |fp32 evaluation - fp64| of that conv (+ of the skip term), + two_rounding_slack where
    the skip term is rounded to bf16 before the add.  Accumulation in less than fp32 would show."""
    c = RR.case(id_, B, h, cin, cout, rs=rs, skip=skip, tm=tm, tn=tn)
    plan = RR.plan_of(c)
    RR.expect_plan(plan, want)
    g = torch.Generator().manual_seed(900 + cin + h)
    t = _gauss_inputs(300 + cin + h, B, h, cin, "rows")
    a_obs, _ = probe(O, L, B, h, cin, 32, rs, t, True, 1e-5)
    ho = plan.ho
    t["w"] = (torch.randn(cout, 9 * cin, generator=g) / (3 * cin ** 0.5)).to(BF16)
    t["bias"] = 0.1 * torch.randn(cout, generator=g)
    kw = {}
    if skip and skip[0] == "conv":
        kw = dict(xskip=torch.randn(B * ho * ho, skip[1], generator=g).to(BF16),
                  wskip=(torch.randn(cout, skip[1], generator=g) / skip[1] ** 0.5).to(BF16),
                  bskip=0.1 * torch.randn(cout, generator=g) if skip[2] else None)
    elif skip:
        hr = ho // 2 if skip[1] == UP2 else 2 * ho if skip[1] == DOWN2 else ho
        kw = dict(resid=torch.randn(B * hr * hr, cout, generator=g).to(BF16), resid_resample=skip[1])
    t.update(kw)
    out = launch(O, L, plan, B, h, cin, cout, t, rs=rs, tm=tm, tn=tn)
    o64, o32 = [RR.resconv_ref(t["x"], B, h, t["w"], t["gamma"], t["beta"], 1e-5, bias=t["bias"], resample=rs,
                               dtype=dt, act=a_obs, **kw) for dt in (F64, F32)]
    floor = R.floor_of(o32["conv"], o64["conv"])
    slack = torch.zeros_like(o64["y"])
    if o64["skip_pre"] is not None:
        fs = R.floor_of(o32["skip_pre"], o64["skip_pre"])
        floor += fs
        slack = N.two_rounding_slack(o64["skip_pre"], fs)
    err = (out.double() - o64["y"]).abs()
    ex = (err - (2.0 ** -7 * o64["y"].abs() + floor + slack)).max().item()
    print(f"{id_}: floor {floor:.3e} max|out-ref| {err.max().item():.3e} excess {ex:.3e}")
    assert ex <= 0, f"{id_}: an element exceeds 2^-7 |ref| + {floor:.3e} by {ex:.3e}"


# ====================================================================== (d) refusals
@pytest.mark.parametrize("id_,kw,code", RR.REFUSALS, ids=[r[0] for r in RR.REFUSALS])
def test_refusals(O, L, id_, kw, code):
    """Each line of rc_plan refuses before anything is launched: the query and the launch return the
    plan copy's code, ops.resconv_fwd gives False (shape / unsupported) or raises (argument), and y
    keeps every sentinel."""
    assert RR.RcPlan(**kw).rc == code
    k = dict(groups=32, resample=NONE, film=False, ld_film=0, film_addr=0, cskip=0, resid=False, resid_resample=NONE,
             tile_m=0, tile_n=0)
    k.update(kw)
    B, h, cin, cout = k["batch"], k["h"], k["cin"], k["cout"]
    ho = 2 * h if k["resample"] == UP2 else h // 2 if k["resample"] == DOWN2 else h
    x = torch.zeros(B * h * h, cin, dtype=BF16, device=dev)
    w = torch.zeros(cout, 9 * cin, dtype=BF16, device=dev)
    gamma, beta = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    fbuf = torch.zeros(B * max(k["ld_film"], 2 * cin) + 8, device=dev)
    film = fbuf[k["film_addr"] // 4:] if k["film"] else None
    y = Guard(max(B * ho * ho, 1), cout, BF16, strided=True)
    resid = torch.zeros(B * 4 * ho * ho + 4, cout, dtype=BF16, device=dev) if k["resid"] else None
    xs = torch.zeros(B * ho * ho, k["cskip"], dtype=BF16, device=dev) if k["cskip"] else None
    ws = torch.zeros(cout, k["cskip"], dtype=BF16, device=dev) if k["cskip"] else None
    a = L.ResConvArgs(batch=B, h=h, cin=cin, cout=cout, resample=k["resample"], groups=k["groups"], silu=1, eps=1e-5,
                      x=_ptr(x), ld_x=cin, gamma=_ptr(gamma), beta=_ptr(beta), film=_ptr(film), ld_film=k["ld_film"],
                      w=_ptr(w), ld_w=9 * cin, y=_ptr(y.view), ld_y=y.view.stride(0), resid=_ptr(resid), ld_resid=cout,
                      resid_resample=k["resid_resample"], cskip=k["cskip"], xskip=_ptr(xs), ld_xskip=k["cskip"],
                      wskip=_ptr(ws), ld_wskip=k["cskip"], tile_m=k["tile_m"], tile_n=k["tile_n"])
    assert L.lib.encdiff_resconv_query(ctypes.byref(a), None, None) == code
    assert L.lib.encdiff_resconv_fwd(ctypes.byref(a), _stream()) == code
    old = O.RC_TILE_M, O.RC_TILE_N
    O.RC_TILE_M, O.RC_TILE_N = k["tile_m"], k["tile_n"]
    try:
        call = lambda: O.resconv_fwd(x, O.Geom(B, h, h), w, y.view, gamma, beta, 1e-5, film=film,  # noqa: E731
                                     ld_film=k["ld_film"], resample=k["resample"], resid=resid,
                                     resid_resample=k["resid_resample"], xskip=xs, wskip=ws, groups=k["groups"])
        if code == RR.ERR_ARG:
            with pytest.raises(L.HipError):
                call()
        else:
            assert call() is False
    finally:
        O.RC_TILE_M, O.RC_TILE_N = old
    torch.cuda.synchronize()
    y.check()
    assert R.same_bits(y.view, y.before.as_strided(*y.geom)), "a refused launch wrote y"
