"""CPU checks of tests/resconv_restate.py, the reference and plan copy of
tests/test_gpu_resconv_paths.py: the reference is held against torch.nn.functional in fp64 for every
option, so that a wrong reference cannot make a wrong kernel pass; the two-valued builder's three
exactness conditions are checked on every parameter set the GPU file uses (the same case table,
imported); the plan copy is checked for its invariants over the whole accepted domain."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import resconv_restate as RR
from resconv_restate import DOWN2, NONE, UP2

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _nchw(rows, B, h):
    return rows.reshape(B, h, h, -1).permute(0, 3, 1, 2)


def _rows(nchw):
    return nchw.permute(0, 2, 3, 1).reshape(-1, nchw.shape[1])


def _bf(t):
    return t.to(BF16).double()


REF_CASES = [  # (B, h, cin, cout, groups, rs, film, silu, bias, skip)
    (2, 4, 64, 16, 32, NONE, "rows", True, True, ("resid", NONE)),
    (2, 4, 32, 16, 8, DOWN2, "one", True, False, ("resid", DOWN2)),
    (4, 2, 64, 32, 32, UP2, None, False, True, ("resid", UP2)),
    (2, 6, 32, 16, 32, UP2, "rows", False, True, ("conv", 32, True)),
    (3, 4, 96, 16, 32, NONE, None, True, True, ("conv", 64, False)),
    (2, 1, 64, 16, 64, NONE, "rows", True, True, None),
    (2, 2, 64, 16, 32, DOWN2, None, True, True, None),
]


@pytest.mark.parametrize("B,h,cin,cout,groups,rs,film,silu,bias,skip", REF_CASES)
def test_reference_matches_functional(B, h, cin, cout, groups, rs, film, silu, bias, skip):
    """resconv_ref in fp64 against F.group_norm / F.silu / F.avg_pool2d / F.interpolate / F.conv2d
    with the same rounding points.  A swapped scale / shift half, a transposed tap, padding at the
    wrong resolution, a pool of the unrounded activation or a skip added before its rounding shows."""
    g = torch.Generator().manual_seed(B * 100 + h * 10 + cin)
    ho = 2 * h if rs == UP2 else h // 2 if rs == DOWN2 else h
    x = (torch.randn(B * h * h, cin, generator=g) * 1.5 + 0.3).to(BF16)
    gamma = (1 + 0.3 * torch.randn(cin, generator=g))
    beta = 0.3 * torch.randn(cin, generator=g)
    E = {None: None, "rows": 0.3 * torch.randn(B, 2 * cin + 32, generator=g),
         "one": 0.3 * torch.randn(1, 2 * cin, generator=g)}[film]
    w4 = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(BF16)
    w = w4.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()
    b = 0.1 * torch.randn(cout, generator=g) if bias else None
    kw = {}
    if skip and skip[0] == "conv":
        kw = dict(xskip=torch.randn(B * ho * ho, skip[1], generator=g).to(BF16),
                  wskip=(torch.randn(cout, skip[1], generator=g) / skip[1] ** 0.5).to(BF16),
                  bskip=0.1 * torch.randn(cout, generator=g) if skip[2] else None)
    elif skip:
        hr = ho // 2 if skip[1] == UP2 else 2 * ho if skip[1] == DOWN2 else ho
        kw = dict(resid=torch.randn(B * hr * hr, cout, generator=g).to(BF16), resid_resample=skip[1])
    o = RR.resconv_ref(x, B, h, w, gamma, beta, 1e-5, groups=groups, film=E, silu=silu, bias=b, resample=rs, **kw)
    # torch.nn.functional, fp64
    n = F.group_norm(_nchw(x.double(), B, h), groups, gamma.double(), beta.double(), 1e-5)
    if E is not None:
        Ee = E.expand(B, -1).double()
        n = n * (1 + Ee[:, :cin, None, None]) + Ee[:, cin:2 * cin, None, None]
    pre = F.silu(n) if silu else n
    assert (o["pre"] - _rows(pre)).abs().max().item() < 1e-11
    a = _bf(_nchw(o["pre"], B, h))  # rounded from the restatement's own value: no flips between the two
    if rs == DOWN2:
        a = _bf(F.avg_pool2d(a, 2))
    elif rs == UP2:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    assert torch.equal(_rows(a), o["a"])
    y = F.conv2d(a, w4.double(), None if b is None else b.double(), padding=1)
    assert (o["conv"] - _rows(y)).abs().max().item() < 1e-11
    if "xskip" in kw:
        s = F.conv2d(_nchw(kw["xskip"].double(), B, ho), kw["wskip"].double()[:, :, None, None],
                     None if kw["bskip"] is None else kw["bskip"].double())
        assert (o["skip_pre"] - _rows(s)).abs().max().item() < 1e-11
        y = y + _nchw(_bf(o["skip_pre"]), B, ho)
    elif "resid" in kw:
        hr = kw["resid"].shape[0] // B
        r = _nchw(kw["resid"].double(), B, int(round(hr ** 0.5)))
        if skip[1] == DOWN2:
            r = _bf(F.avg_pool2d(r, 2))
        elif skip[1] == UP2:
            r = F.interpolate(r, scale_factor=2, mode="nearest")
        y = y + r
    assert (o["y"] - _rows(y)).abs().max().item() < 1e-11
    assert torch.equal(o["out"], o["y"].to(BF16))


def test_pool_order_and_neighbours():
    """The pool adds ((a + b) + c + d) / 4 (visible in fp32 on values 2^24 apart); bf16 neighbours and
    rounding-boundary distances at a power of two, where the ulp changes."""
    s = torch.tensor([[2.0 ** 24], [1.0], [1.0], [-2.0 ** 24]], dtype=F32)  # one image of 2x2, one channel
    assert RR.pool_kernel_order(s, 1, 1).item() == 0.0       # ((2^24 + 1) + 1) - 2^24 in fp32: the ones are lost
    assert RR.pool_kernel_order(s.double(), 1, 1).item() == 0.5
    lo, hi = RR.bf16_neighbours(torch.tensor([1.0, -1.0, 1.5], dtype=BF16))
    assert lo.tolist() == [1 - 2.0 ** -8, -1 - 2.0 ** -7, 1.5 - 2.0 ** -7]
    assert hi.tolist() == [1 + 2.0 ** -7, -1 + 2.0 ** -8, 1.5 + 2.0 ** -7]
    d = RR.boundary_distance(torch.tensor([1.0, 1.0 + 2.0 ** -9, 1.0 - 2.0 ** -10, -3.0], dtype=F64))
    assert d.tolist() == [2.0 ** -9, 2.0 ** -9, 2.0 ** -10, 2.0 ** -7]
    assert RR.quantum(torch.tensor([0.0, 1.5, -0.375, 6.0])) == 0.125
    assert RR.quantum(torch.tensor([1 + 2.0 ** -7])) == 2.0 ** -7


def test_lattice_counts():
    """How much of the lattice the margin leaves (both signs of x counted): 550 of 600 (combination,
    sign) pairs with SiLU, 556 without -- the 44 lost there are the z = 0 ones, whose true value is
    the residue +-mul (1 - rstd), far below the fp32 error of mul.  The derived fp32 slack is far
    below the margin on everything that passes."""
    for silu, n in ((True, 550), (False, 556)):
        ok, count, ratio = RR.lattice_table(1e-5, silu)
        print(f"silu {silu}: {count} of 600 pass, smallest distance / derived slack {ratio:.1f}")
        assert count == n
        assert ratio > 8
    ok, count, _ = RR.lattice_table(1e-5, True, RR.ZR_SILU)
    assert ok.sum() >= 50  # the range cut of the wide-cin cases leaves a comfortable set


@pytest.mark.parametrize("c", RR.EXACT_CASES, ids=[c.id for c in RR.EXACT_CASES])
def test_exact_case_conditions(c):
    """Every exact case of the GPU file: the plan it asserts, x balanced per (image, group), and the
    three conditions -- (a) every true activation clear of the bf16 rounding boundaries by the margin
    and by the derived fp32 slack, (b) the conv's input rows multiples of q, (c) sum |w| |a| / q below
    2^24 for the conv, the skip conv and the pool."""
    RR.expect_plan(RR.plan_of(c), c.want)
    t = RR.exact_inputs(c)
    v = t["x"].double().reshape(c.B, c.h * c.h, c.groups, -1)
    assert (v.abs() == 1).all() and (v.sum(dim=(1, 3)) == 0).all()
    ref = RR.exact_reference(c, t)
    cond = RR.exact_conditions(c, t, ref)
    print(c.id, cond)
    RR.assert_exact_conditions(cond)
    m, r = RR.N.gn_stats_onepass(t["x"], c.B, c.h * c.h, c.groups, c.eps)
    assert (m == 0).all() and (r == RR.rstd_two_valued(c.eps)).all()
    assert torch.isfinite(ref["out"].float()).all() and ref["out"].float().abs().max() > 0


def test_case_tables_reach_their_paths():
    """The Gaussian cases' plan facts and every refusal's code, on the CPU copy of the plan."""
    for id_, B, h, cin, groups, rs, want in RR.PROBE_CASES:
        RR.expect_plan(RR.RcPlan(B, h, cin, cin, resample=rs, groups=groups), want)
    for id_, B, h, cin, cout, rs, skip, tm, tn, want in RR.CONTRACT_CASES:
        c = RR.case(id_, B, h, cin, cout, rs=rs, skip=skip, tm=tm, tn=tn)
        RR.expect_plan(RR.plan_of(c), want)
    for id_, kw, code in RR.REFUSALS:
        assert RR.RcPlan(**kw).rc == code, id_
    # what the exact table must reach between its cases
    P = [RR.plan_of(c) for c in RR.EXACT_CASES]
    assert {p.ipw for p in P} == {1, 4, 16}
    assert {p.mc for p in P} == {1, 2, 4} and {p.wk for p in P} == {2, 4, 8}
    assert {p.xcd_remap for p in P} == {True, False}
    assert {p.streamed for p in P} == {True, False} and any(0 < p.kl < p.KS for p in P) and any(p.kl == 0 for p in P)
    assert any(p.empty_waves for p in P) and any(p.midtap_starts for p in P)
    assert {p.mtg for p in P} >= {1, 4, 9, 16, 25}


def _domain():
    for h, cin in itertools.product(range(1, 33), range(32, 513, 32)):
        for cout, B, rs, tm, tn in itertools.product((16, 64, 256), (1, 4, 8, 16, 32), (NONE, DOWN2, UP2),
                                                     (0, 1, 2, 4), (0, 1, 2)):
            yield dict(batch=B, h=h, cin=cin, cout=cout, resample=rs, tile_m=tm, tile_n=tn)


def _check_invariants(p, kw):
    assert p.nchunk * p.mc == p.mtg, f"tiles without a workgroup: {kw} mc {p.mc} mtg {p.mtg}"
    assert p.mc * p.wk == RR.RC_NW
    ks = p.kranges
    assert ks[0][0] == 0 and ks[-1][1] == p.KS and all(a[1] == b[0] for a, b in zip(ks, ks[1:])), (kw, ks)
    assert all(a <= b for a, b in ks)
    assert p.kl % 2 == 0 or p.kl == p.KS, (kw, p.kl)
    assert 0 <= p.kl <= p.KS and p.lds <= 160 * 1024
    assert p.grid == p.nslice * p.ngroup * p.nchunk
    assert p.lpi >= 1 and 0 <= p.idle < RR.RC_THREADS


def test_plan_invariants_over_domain():
    """Over h 1..32, cin 32..512, three couts, five batches, the three resamples and every tile
    override: whatever the plan accepts gives every 16-row tile a workgroup (nchunk * mc == mtg), k
    ranges that tile [0, KS), an even kl (or all of KS) and at most 160 KiB of LDS."""
    n = 0
    for kw in _domain():
        p = RR.RcPlan(**kw)
        if p.ok:
            n += 1
            _check_invariants(p, kw)
    assert n > 50000


def test_heuristic_defect_stated():
    """The heuristic before the largest-divisor rule: 12x12 (mtg = 9) at B = 8, cout = 256 kept mc = 4,
    two chunks, and left tile 8 of every image (output rows 128..143) without a workgroup.  The rule
    does not change a plan whose mtg is 1, 4, 16 or 64."""
    old = RR.RcPlan(8, 12, 32, 256, divisor_fix=False)
    assert (old.mc, old.nchunk, old.mtg) == (4, 2, 9)
    new = RR.RcPlan(8, 12, 32, 256)
    assert (new.mc, new.nchunk) == (1, 9)
    for kw in _domain():
        a, b = RR.RcPlan(**kw), RR.RcPlan(divisor_fix=False, **kw)
        if a.ok and a.mtg in (1, 4, 16, 64):
            assert (a.mc, a.nchunk, a.kl, a.lds, a.grid) == (b.mc, b.nchunk, b.kl, b.lds, b.grid), kw
