"""CPU checks of tests/elementwise_restate.py, the references of tests/test_gpu_elementwise.py:
each restatement is held against an independent torch formulation, so that a wrong reference
cannot make a wrong kernel pass (or a right one fail)."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_restate as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def test_split_bf16_reproduces_the_weight():
    """hi + lo == w to 2^-16 |w| (a lo formed from the wrong residual, or hi truncated instead of
    rounded to nearest even, breaks this)."""
    torch.manual_seed(0)
    w = torch.cat([torch.randn(4096) * 3, torch.tensor([0.0, -0.0, 1.0, 1.00390625, 255.5, 1e-20, -3e20])])
    hi, lo = R.split_bf16(w)
    assert hi.dtype == BF16 and lo.dtype == BF16
    assert torch.equal(hi, w.to(BF16))
    err = (hi.double() + lo.double() - w.double()).abs()
    assert (err <= 2.0 ** -16 * w.double().abs()).all()


def test_pack_kind0_and_kind6():
    """kind 0 is the cast, kind 6 equals .t()."""
    torch.manual_seed(1)
    src = torch.randn(5000)
    assert torch.equal(R.pack_ref(src, 8, 10, 20, 0), src[8:208].to(BF16))
    for rows, cols in [(32, 32), (70, 45), (1, 129)]:
        got = R.pack_ref(src, 3, rows, cols, 6).view(cols, rows)
        assert torch.equal(got, src[3:3 + rows * cols].view(rows, cols).t().to(BF16))


def test_pack_kind1_is_channels_last():
    """kind 1 equals permute(0, 2, 3, 1) of the [co][ci][3][3] weight."""
    torch.manual_seed(2)
    for co, cin in [(32, 16), (7, 5)]:
        w = torch.randn(co, cin, 3, 3)
        got = R.pack_ref(w.reshape(-1), 0, co, 9 * cin, 1, cin).view(co, 3, 3, cin)
        assert torch.equal(got, w.permute(0, 2, 3, 1).to(BF16))
        # as the GEMM B operand it reproduces the convolution: [co][tap][ci] . im2col
        x = torch.randn(1, cin, 5, 5).to(BF16).float()
        cols = F.unfold(x, 3, padding=1).view(cin, 9, 25).permute(1, 0, 2).reshape(9 * cin, 25)
        y = got.float().reshape(co, 9 * cin) @ cols
        assert torch.allclose(y.view(1, co, 5, 5), F.conv2d(x, w.to(BF16).float(), padding=1), atol=1e-3)


@pytest.mark.parametrize("cin,taps", [(3, 9), (3, 16), (8, 9)])
def test_pack_kind2_pads_channels(cin, taps):
    """kind 2: [co][cin][taps] -> [co][tap][8]; channels cin..7 are zero, the rest a permute."""
    torch.manual_seed(3)
    co = 6
    w = torch.randn(co, cin, taps)
    got = R.pack_ref(w.reshape(-1), 0, co, 8 * taps, 2, cin).view(co, taps, 8)
    assert torch.equal(got[:, :, :cin], w.permute(0, 2, 1).to(BF16))
    assert (got[:, :, cin:] == 0).all()


def test_pack_split_kinds():
    """kinds 3 / 4 / 5: block order [hi | hi | lo] (kind 5: + [I | I]); swapped hi / lo blocks or a
    transposed identity break these."""
    torch.manual_seed(4)
    co, cin, taps = 5, 24, 16
    w = torch.randn(co, taps, cin)
    got = R.pack_ref(w.reshape(-1), 0, co, 3 * cin * taps, 3, cin).view(co, taps, 3, cin)
    hi, lo = R.split_bf16(w)
    assert torch.equal(got[:, :, 0], hi) and torch.equal(got[:, :, 1], hi) and torch.equal(got[:, :, 2], lo)
    co, cin, taps = 4, 3, 16
    w = torch.randn(co, cin, taps)
    got = R.pack_ref(w.reshape(-1), 0, co, 24 * taps, 4, cin).view(co, taps, 3, 8)
    hi, lo = R.split_bf16(w.permute(0, 2, 1))
    assert torch.equal(got[:, :, 0, :cin], hi) and torch.equal(got[:, :, 1, :cin], hi)
    assert torch.equal(got[:, :, 2, :cin], lo) and (got[:, :, :, cin:] == 0).all()
    for c in (32, 128):
        w = torch.randn(c, c)
        got = R.pack_ref(w.reshape(-1), 0, c, 5 * c, 5, c).view(c, 5, c)
        hi, lo = R.split_bf16(w)
        assert torch.equal(got[:, 0], hi) and torch.equal(got[:, 1], hi) and torch.equal(got[:, 2], lo)
        assert torch.equal(got[:, 3].float(), torch.eye(c)) and torch.equal(got[:, 4].float(), torch.eye(c))
        # the operand's purpose: [a_hi | a_lo | a_hi | x_hi | x_lo] . row == a w + x to ~2^-16
        a = torch.randn(c)
        ah, al = R.split_bf16(a)
        act = torch.cat([ah, al, ah, ah, al]).double()
        y = got.reshape(c, 5 * c).double() @ act
        ref = w.double() @ a.double() + a.double()
        assert (y - ref).abs().max() <= 2.0 ** -14 * (w.abs().double() @ a.abs().double() + a.abs().double()).max()
    assert R.pack_src_elems(5, 3 * 24 * 16, 3, 24) == 5 * 16 * 24
    assert R.pack_src_elems(4, 24 * 16, 4, 3) == 4 * 3 * 16


def test_layout_restatements():
    """nchw_to_rows == permute + zero padding, split3 blocks [hi | lo | hi], fp32 round trip."""
    torch.manual_seed(5)
    B, C, HW, cpad = 3, 4, 10, 8
    x = torch.randn(B, C, HW)
    r = R.nchw_to_rows_ref(x, cpad)
    assert r.shape == (B * HW, cpad) and (r[:, C:] == 0).all()
    assert torch.equal(r[:, :C].view(B, HW, C), x.transpose(1, 2).to(BF16))
    s = R.nchw_to_rows_ref(x, cpad, split=True)
    hi, lo = R.split_bf16(R.nchw_rows_f32_ref(x, cpad))
    assert torch.equal(s[:, :cpad], hi) and torch.equal(s[:, cpad:2 * cpad], lo) and torch.equal(s[:, 2 * cpad:], hi)
    assert torch.equal(R.rows_to_nchw_ref(R.nchw_rows_f32_ref(x, cpad), B, C, HW), x)


def test_resample_restatements():
    """avg-pool / nearest and their adjoints against torch's own ops and autograd."""
    torch.manual_seed(6)
    b, h, w, c = 2, 6, 4, 5
    nchw = lambda r, hh, ww: r.reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    x = torch.randn(b * 4 * h * w, c, dtype=F64, requires_grad=True)
    y = R.avgpool2(x, b, h, w)
    assert torch.allclose(nchw(y, h, w), F.avg_pool2d(nchw(x, 2 * h, 2 * w), 2), atol=1e-14)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert torch.allclose(R.avgpool2_adjoint(dy, b, 2 * h, 2 * w), x.grad, atol=1e-14)
    xs = torch.randn(b * (h // 2) * (w // 2), c, dtype=F64, requires_grad=True)
    yu = R.nearest2(xs, b, h, w)
    assert torch.equal(nchw(yu, h, w), F.interpolate(nchw(xs, h // 2, w // 2), scale_factor=2, mode="nearest"))
    du = torch.randn_like(yu)
    yu.backward(du)
    assert torch.allclose(R.nearest2_adjoint(du, b, h // 2, w // 2), xs.grad, atol=1e-14)


def test_activation_restatements():
    """SiLU / GELU and their derivatives against torch and autograd in fp64."""
    x = torch.linspace(-30, 30, 4001, dtype=F64, requires_grad=True)
    assert torch.allclose(R.silu(x), F.silu(x), atol=1e-15)
    assert torch.allclose(R.gelu(x), F.gelu(x), atol=1e-15)
    (gs,) = torch.autograd.grad(F.silu(x).sum(), x)
    assert torch.allclose(R.silu_grad(x), gs, atol=1e-14)
    (gg,) = torch.autograd.grad(F.gelu(x).sum(), x)
    assert torch.allclose(R.gelu_grad(x), gg, atol=1e-14)
    f = torch.randn(7, 16, dtype=F64, requires_grad=True)
    dy = torch.randn(7, 8, dtype=F64)
    a, g = f.chunk(2, -1)
    (a * F.gelu(g)).backward(dy)
    assert torch.allclose(R.geglu(f), a * F.gelu(g)) and torch.allclose(R.geglu_bwd(f, dy), f.grad, atol=1e-14)


def test_adamw_ema_restatement_matches_torch_optim():
    """adamw_ema_step in fp64 == torch.optim.AdamW + LitEma's rule over three steps, nonzero decay."""
    from oracle import encdiff_oracle as OR
    from encdiff_amd.ops import adamw_hyper  # host scalars only
    torch.manual_seed(7)
    n, ema_n = 64, 41
    p0 = torch.randn(n, dtype=F64)
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([par], lr=1e-3, weight_decay=0.05)
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    ema = p0.clone()
    rema = p0.clone()
    for step in (1, 2, 3):
        g = torch.randn(n, dtype=F64)
        g[::7] = 0
        par.grad = g.clone()
        opt.step()
        omd = 1 - min(0.9999, (1 + step) / (10 + step))
        rema[:ema_n] -= omd * (rema[:ema_n] - par.detach()[:ema_n])
        hy = torch.tensor(adamw_hyper(1e-3, step, weight_decay=0.05, ema_one_minus_decay=omd), dtype=F64)
        p, m, v, ema = R.adamw_ema_step(p, g, m, v, ema, ema_n, hy)
        assert torch.allclose(p, par.detach(), rtol=1e-12, atol=1e-15)
        assert torch.allclose(ema, rema, rtol=1e-12, atol=1e-15)
    assert torch.equal(ema[ema_n:], p0[ema_n:])
    # and the repository's oracle agrees (default weight decay)
    rp, rm, rv = OR.adamw_step(p0, g, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), 1, 1e-3)
    hy = torch.tensor(adamw_hyper(1e-3, 1), dtype=F64)
    q, qm, qv, _ = R.adamw_ema_step(p0, g, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), None, 0, hy)
    assert torch.allclose(q, rp, rtol=1e-12) and torch.allclose(qm, rm) and torch.allclose(qv, rv)


def test_diffusion_restatements():
    """Timestep embedding, q_sample, DDIM step and L1 against the oracle's fp32 forms."""
    from oracle import encdiff_oracle as OR
    torch.manual_seed(8)
    t = torch.tensor([0, 1, 2, 500, 998, 999])
    for dim in (64, 128, 256):
        e64 = R.timestep_embedding(t, dim)
        assert (e64.float() - OR.timestep_embedding(t, dim)).abs().max() < 2e-4
        assert torch.equal(e64[0, :dim // 2], torch.ones(dim // 2, dtype=F64)) and (e64[0, dim // 2:] == 0).all()
    sch = OR.sched_fp32(OR.register_schedule())
    B, per = 6, 48
    x0, eps = torch.randn(B, per), torch.randn(B, per)
    xt = R.q_sample(x0, eps, t, sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"])
    ref = OR.q_sample(sch, x0.view(B, 3, 4, 4), t, eps.view(B, 3, 4, 4)).view(B, per)
    assert (xt.float() - ref).abs().max() < 1e-6
    sc = torch.tensor([0.37])
    xs = R.q_sample(x0, eps, t, sch["sqrt_alphas_cumprod"], sch["sqrt_one_minus_alphas_cumprod"], scale=sc)
    ref = OR.q_sample(sch, 0.37 * x0.view(B, 3, 4, 4), t, eps.view(B, 3, 4, 4)).view(B, per)
    assert (xs.float() - ref).abs().max() < 1e-6
    z = torch.randn(B, per)
    xp, p0 = R.ddim_step(xt.float(), eps, z, 0.5, 0.7, 0.1, math.sqrt(0.5))
    rx, rp = OR.ddim_step(xt.float(), eps, 0.5, 0.7, 0.1, math.sqrt(0.5), z)
    assert (xp.float() - rx).abs().max() < 1e-5 and (p0.float() - rp).abs().max() < 1e-5
    xp0, _ = R.ddim_step(xt.float(), eps, None, 0.5, 0.7, 0.1, math.sqrt(0.5))
    assert torch.allclose(xp0 + torch.tensor(0.1, dtype=F32).double() * z.double(), xp)
    pred = torch.randn(B, per)
    pred[0, :5] = eps[0, :5]
    loss, vlb, ls = R.l1_loss(pred, eps, t, sch["lvlb_weights"], 0.25)
    rl, d = OR.p_losses_from_output(sch, pred.view(B, 3, 4, 4), eps.view(B, 3, 4, 4), t, l_simple_weight=0.25)
    assert abs(loss.item() - rl.item()) < 1e-6 and abs(vlb.item() - d["loss_vlb"].item()) < 1e-6 * max(1, vlb.item())
    gr = R.l1_grad(pred, eps, 0.25)
    assert (gr[0, :5] == 0).all() and set(gr.abs().unique().tolist()) == {0.0, gr.abs().max().item()}
    pr = pred.clone().requires_grad_(True)
    (0.25 * (eps - pr).abs().mean(1).mean()).backward()
    assert torch.allclose(gr, pr.grad, rtol=1e-6, atol=0)


def test_grad_fold_and_batchnorm_restatements():
    """grad_fold == gw + dw.permute over the live channels; BatchNorm == nn.BatchNorm2d in fp64."""
    torch.manual_seed(9)
    co, cin, cpad, taps = 4, 3, 8, 9
    dw = torch.randn(co * taps * cpad)
    gw = torch.randn(co * cin * taps)
    out = R.grad_fold_ref(gw, dw, co, cin, cpad, taps)
    for o, c, t in [(0, 0, 0), (3, 2, 8), (1, 2, 4)]:
        assert out[o, c, t] == gw[(o * cin + c) * taps + t] + dw[(o * taps + t) * cpad + c]
    rows, C = 50, 8
    x = torch.randn(rows, C) * 2 + 0.5
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    ref = torch.relu(bn(x.double().t().reshape(1, C, rows, 1))).reshape(C, rows).t()
    y, mean, rstd = R.batchnorm_train(x, gamma, beta, 1e-5, True)
    assert torch.allclose(y, ref, atol=1e-12)
    assert torch.allclose(R.batchnorm_apply(x, mean, rstd, gamma, beta, True), y, atol=1e-12)


def test_comparison_rules():
    """The rules reject one bad element in a large tensor (what whole-tensor rel-L2 cannot see)."""
    ref = torch.randn(4096, dtype=F64)
    out = ref.to(BF16)
    assert R.bf16_excess(out, ref, 0.0)[0] <= 0
    bad = out.clone()
    bad[4095] = bad[4095] * 1.02 + 0.01
    ex, i, _ = R.bf16_excess(bad, ref, 0.0)
    assert ex > 0 and i == 4095
    o32 = ref.float()
    assert R.f32_excess(o32, ref, 0.0)[0] <= 0
    b32 = o32.clone()
    b32[7] *= 1 + 2.0 ** -20
    assert R.f32_excess(b32, ref, 0.0)[0] > 0 or b32[7] == 0
    assert R.same_bits(torch.tensor([0.0]), torch.tensor([0.0])) and not R.same_bits(torch.tensor([0.0]),
                                                                                    torch.tensor([-0.0]))
