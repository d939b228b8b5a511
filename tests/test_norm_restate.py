"""CPU checks of tests/norm_restate.py, the references of tests/test_gpu_norm.py: every restatement
is held against torch's own GroupNorm / LayerNorm / pooling autograd in fp64, so that a wrong
reference cannot make a wrong kernel pass (or a right one fail); the copy of the slice heuristic is
held against a table worked out by hand from the rule in csrc/norm.hip."""
import pytest
import torch
import torch.nn.functional as F

import norm_restate as N

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _nchw(rows, B, h, w):
    return rows.reshape(B, h, w, -1).permute(0, 3, 1, 2)


def _rows(nchw):
    return nchw.permute(0, 2, 3, 1).reshape(-1, nchw.shape[1])


def _close(a, b, tol=1e-11):
    scale = max(1.0, b.abs().max().item())
    assert (a - b).abs().max().item() <= tol * scale, (a - b).abs().max().item()


GN_CASES = [(64, 4, 4, 2, 32, True, True), (96, 3, 5, 2, 32, False, True), (32, 8, 8, 3, 32, True, False),
            (64, 2, 2, 2, 8, True, True), (128, 1, 1, 2, 32, False, False)]


@pytest.mark.parametrize("C,h,w,B,G,film,silu", GN_CASES)
def test_groupnorm_restatement_matches_autograd(C, h, w, B, G, film, silu):
    """Forward (one-pass and two-pass statistics, y, silu'(z)) and the backward from given
    statistics (dx, per-image d gamma / d beta, d scale / d shift) against F.group_norm autograd in
    fp64.  A swapped scale / shift half, a group mean over the wrong count, FiLM applied before
    the affine, or d gamma summed over dz instead of dn shows here."""
    g = torch.Generator().manual_seed(C + h)
    HW = h * w
    x = (torch.randn(B * HW, C, generator=g) * 2 + 0.5).to(BF16)
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).double()
    beta = (0.3 * torch.randn(C, generator=g)).double()
    E = (torch.randn(B, 2 * C + 32, generator=g) * 0.3).double() if film else None
    dy = torch.randn(B * HW, C, generator=g).to(BF16)
    eps = 1e-5
    xr = _nchw(x.double(), B, h, w).clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    Er = E.clone().requires_grad_(True) if film else None
    z = F.group_norm(xr, G, gr, br, eps)
    if film:
        z = z * (1 + Er[:, :C, None, None]) + Er[:, C:2 * C, None, None]
    ref = F.silu(z) if silu else z
    ref.backward(_nchw(dy.double(), B, h, w))

    m1, r1 = N.gn_stats_onepass(x, B, HW, G, eps)
    m2, r2 = N.gn_stats_twopass(x, B, HW, G, eps)
    _close(m1, m2)
    _close(r1, r2, 1e-9)
    y, ds = N.gn_apply(x, B, HW, gamma, beta, m2, r2, film=E, use_silu=silu)
    _close(y, _rows(ref.detach()), 1e-9)
    if silu:
        zz = _rows(z.detach())
        _close(ds, torch.autograd.functional.jvp(F.silu, zz, torch.ones_like(zz))[1], 1e-9)
    o = N.gn_bwd(x, B, HW, gamma, beta, m2, r2, dy, film=E, use_silu=silu)
    _close(o["dx"], _rows(xr.grad), 1e-8)
    _close(o["dgamma"].sum(0), gr.grad, 1e-9)
    _close(o["dbeta"].sum(0), br.grad, 1e-9)
    if film:
        _close(o["dscale"], Er.grad[:, :C], 1e-9)
        _close(o["dshift"], Er.grad[:, C:2 * C], 1e-9)
        assert Er.grad[:, 2 * C:].abs().max() == 0
    # options: dsilu read instead of recomputed (exact rows -> same result), accumulate, resid, both
    if silu:
        o2 = N.gn_bwd(x, B, HW, gamma, beta, m2, r2, dy, film=E, use_silu=True, dsilu=ds)
        _close(o2["dx"], o["dx"], 1e-12)
    prev = torch.randn(B * HW, C, generator=g).to(BF16)
    res = torch.randn(B * HW, C, generator=g).to(BF16)
    o3 = N.gn_bwd(x, B, HW, gamma, beta, m2, r2, dy, film=E, use_silu=silu, prev=prev, resid=res)
    _close(o3["dx"], o["dx"] + prev.double() + res.double(), 1e-12)


def test_segment_stats_layout_and_statistics():
    """The in_stats helper: element [(2 (b nseg + sg) + k) ld + c] is segment sg's sum (k = 0) / sum
    of squares (k = 1) of channel c, padding columns untouched; the statistics formed from them equal
    the direct ones."""
    g = torch.Generator().manual_seed(5)
    B, HW, C, ld = 3, 128, 48, 56
    x = torch.randn(B * HW, C, generator=g).to(BF16)
    st = N.segment_stats(x, B, HW, ld)
    assert st.shape == (2 * B * 2, ld) and st.dtype == F32 and torch.isnan(st[:, C:]).all()
    b, sg, c = 2, 1, 17
    seg = x[b * HW + 64 * sg: b * HW + 64 * sg + 64, c].double()
    flat = st.reshape(-1)
    assert flat[(2 * (b * 2 + sg) + 0) * ld + c] == seg.sum().float()
    assert flat[(2 * (b * 2 + sg) + 1) * ld + c] == (seg * seg).sum().float()
    m, r = N.gn_stats_from_segments(st, B, HW, C, 8, 1e-5)
    m0, r0 = N.gn_stats_twopass(x, B, HW, 8, 1e-5)
    _close(m, m0, 1e-6)
    _close(r, r0, 1e-5)


@pytest.mark.parametrize("B,h,w", [(2, 4, 6), (1, 1, 1), (3, 2, 2)])
def test_resample_adjoints_match_autograd(B, h, w):
    """DOWN2: the adjoint of F.avg_pool2d(2) following an (h, w) tensor; UP2: of nearest x2.
    The restated UP2 sum keeps the order ((a + b) + c) + d."""
    g = torch.Generator().manual_seed(7 + h)
    C = 8
    if h % 2 == 0 and w % 2 == 0:
        t = torch.randn(B * (h // 2) * (w // 2), C, generator=g).to(BF16)
        src = torch.zeros(B, C, h, w, dtype=F64, requires_grad=True)
        F.avg_pool2d(src, 2).backward(_nchw(t.double(), B, h // 2, w // 2))
        _close(N.resample_adjoint(t, N.DOWN2, B, h, w), _rows(src.grad), 1e-15)
    t = torch.randn(B * 4 * h * w, C, generator=g).to(BF16)
    src = torch.zeros(B, C, h, w, dtype=F64, requires_grad=True)
    F.interpolate(src, scale_factor=2, mode="nearest").backward(_nchw(t.double(), B, 2 * h, 2 * w))
    _close(N.resample_adjoint(t, N.UP2, B, h, w), _rows(src.grad), 1e-15)
    # order: children are (row 0: a, b; row 1: c, d); a + (b + (c + d)) would give 1 here
    q = torch.zeros(4, 1, dtype=F32)
    q[0], q[1], q[2], q[3] = 1.0, 2.0 ** 24, -(2.0 ** 24), 0.0
    assert N.resample_adjoint(q, N.UP2, 1, 1, 1, F32).item() == 0.0  # (1 + 2^24) rounds the 1 away first
    # the bf16 dy the kernel uses: one rounding of the fp32 sum
    d = N.resampled_dy(t, N.UP2, B, h, w)
    assert d.dtype == BF16 and torch.equal(d, N.resample_adjoint(t, N.UP2, B, h, w, F32).to(BF16))


def test_gn_bwd_resid_adjoint_is_added_after_rounding():
    """resid_adj is added to the bf16-rounded dx, not to the exact one."""
    g = torch.Generator().manual_seed(9)
    B, HW, C, G = 1, 4, 16, 4
    x = torch.randn(B * HW, C, generator=g).to(BF16)
    dy = torch.randn(B * HW, C, generator=g).to(BF16)
    ra = torch.randn(B * HW, C, generator=g).to(BF16)
    ga, be = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    m, r = N.gn_stats_twopass(x, B, HW, G, 1e-5)
    plain = N.gn_bwd(x, B, HW, ga, be, m, r, dy)["dx"]
    got = N.gn_bwd(x, B, HW, ga, be, m, r, dy, resid_adj=ra)["dx"]
    assert torch.equal(got, plain.to(BF16).double() + ra.double())
    assert not torch.equal(got, plain + ra.double())


@pytest.mark.parametrize("rows,C", [(1, 64), (37, 128), (5, 512)])
def test_layernorm_restatement_matches_autograd(rows, C):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, C, generator=g) + 0.3).to(BF16)
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).double()
    beta = (0.3 * torch.randn(C, generator=g)).double()
    dy = torch.randn(rows, C, generator=g).to(BF16)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (C,), gr, br, 1e-5)
    ref.backward(dy.double())
    y, mean, rstd = N.ln_fwd(x, gamma, beta, 1e-5)
    _close(y, ref.detach(), 1e-10)
    prev = torch.randn(rows, C, generator=g).to(BF16)
    dx, tg, tb = N.ln_bwd(x, gamma, mean, rstd, dy, prev=prev)
    _close(dx - prev.double(), xr.grad, 1e-9)
    owner = N.ln_block_of_rows(rows, C)
    pg, pb = N.partial_rows(tg, owner, N.LN_PARTS), N.partial_rows(tb, owner, N.LN_PARTS)
    _close(pg.sum(0), gr.grad, 1e-10)
    _close(pb.sum(0), br.grad, 1e-10)
    used = torch.zeros(N.LN_PARTS, dtype=torch.bool)
    used[owner] = True
    assert (pg[~used] == 0).all() and (pb[~used] == 0).all()


def test_ln_row_ownership():
    """bf16 backward: block k owns rows {k RPB + rr + j 256 RPB}; fp32: contiguous ranges."""
    assert N.ln_rpb(64) == 32 and N.ln_rpb(128) == 16 and N.ln_rpb(256) == 8 and N.ln_rpb(512) == 4
    o = N.ln_block_of_rows(2 * 256 * 4 + 9, 512)
    assert o[0] == 0 and o[3] == 0 and o[4] == 1 and o[1023] == 255 and o[1024] == 0 and o[2048 + 8] == 2
    o = N.ln_block_of_rows_f32(37, 16)  # per = 3
    assert o[0] == 0 and o[2] == 0 and o[3] == 1 and o[36] == 12


# (C, HW, B) -> cs, from the rule "narrowest multiple of lcm(8, cpg) dividing C with cs * HW >= min_el,
# min_el = (8192 at B >= 64, else 2048) / (1, 2, 4, 8 for HW >= 256, >= 64, >= 16, < 16), else C", groups = 32
SLICE_TABLE = [
    ((64, 256, 2), 8), ((128, 64, 2), 16), ((64, 16, 2), 32), ((64, 4, 2), 64), ((128, 1, 2), 128),
    ((128, 16, 64), 128), ((256, 4, 64), 256), ((512, 1, 64), 512),
    ((96, 64, 2), 24), ((320, 16, 2), 40), ((96, 16, 2), 48), ((320, 4, 2), 80), ((96, 1, 2), 96),
    ((320, 16, 64), 160), ((192, 1, 2), 192), ((320, 1, 2), 320), ((384, 1, 2), 384),
    ((32, 64, 2), 16), ((64, 15, 2), 32), ((64, 4096, 2), 8), ((96, 4096, 2), 24),
    ((64, 64, 2), 16), ((192, 256, 2), 24), ((64, 256, 64), 32),
    ((32, 1024, 2), 8), ((512, 1024, 1), 16), ((128, 1536, 2), 8), ((192, 1024, 2), 24),
    ((640, 1, 64), 640), ((96, 1024, 2), 24), ((192, 169, 64), 48), ((64, 64, 2), 16),
]


@pytest.mark.parametrize("key,cs", SLICE_TABLE, ids=lambda v: str(v))
def test_gn_slice_copy(key, cs):
    C, HW, B = key
    assert N.gn_slice(C, HW, C // 32, B) == cs


def test_gn_slice_groups8():
    """groups = 8 at C = 64: cpg = 8, unit 8."""
    assert N.gn_slice(64, 16, 8, 2) == 32


def test_gn_path_derived_quantities():
    """nvc, np, `one`, tiled, butterfly width and the forward kernel choice for the landmark cases
    of tests/test_gpu_norm.py."""
    p = N.GnPath(512, 1, 64)
    assert (p.nvc, p.np, p.nval, p.red_rows, p.one, p.fwd) == (64, 4, 8, 4, True, "self")
    p = N.GnPath(128, 16, 64)
    assert (p.nvc, p.nval, p.red_rows) == (16, 2, 4)
    p = N.GnPath(256, 4, 64)
    assert (p.nvc, p.nval) == (32, 4)
    p = N.GnPath(64, 4, 2)
    assert (p.nvc, p.nval) == (8, 1)
    p = N.GnPath(192, 1, 2)
    assert (p.nvc, p.np, p.idle, p.pow2) == (24, 10, 16, False)
    assert N.GnPath(320, 1, 2).idle == 16 and N.GnPath(384, 1, 2).idle == 16
    p = N.GnPath(192, 169, 64)
    assert (p.nvc, p.np, p.one, p.bwd_tiled) == (6, 42, False, True)
    p = N.GnPath(96, 1024, 2)
    assert (p.nvc, p.np, p.one, p.bwd_tiled, p.last_batch_partial) == (3, 85, False, False, True)
    assert N.GnPath(96, 4096, 2).fwd_tiled is False and N.GnPath(64, 4096, 2).fwd_tiled is True
    assert N.GnPath(64, 64, 2, in_stats=True).fwd == "stats"
    assert N.GnPath(32, 1024, 2, in_stats=True).fwd == "group_apply"
    assert N.GnPath(512, 1024, 1, in_stats=True).fwd == "group_apply"
    assert N.GnPath(192, 1024, 2, in_stats=True).fwd == "stats"       # 24 vectors do not divide 256
    assert N.GnPath(320, 4096, 1, in_stats=True).fwd == "self"        # 64 segments x 40 channels > 2048
    assert N.GnPath(64, 15, 2, in_stats=True).fwd == "self"           # HW % 64 != 0
    assert not N.GnPath(640, 1, 64).ok and not N.GnPath(36, 4, 2).ok and not N.GnPath(72, 4, 2).ok
    assert N.GnPath(64, 64, 2, slab=True).one is False and N.GnPath(64, 64, 2, slab=True).bwd_tiled
