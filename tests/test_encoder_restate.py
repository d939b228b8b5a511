"""The fp64 restatements of tests/encoder_restate.py against torch autograd in fp64 on the CPU
(1e-12 relative): nn.BatchNorm2d.train() (+ReLU), the as-is Encoder4.warp, View + nn.Linear; and
the arithmetic of the bound helpers."""
import pytest
import torch
from torch import nn

import encoder_restate as E

F64 = torch.float64


def _close(a, b, what):
    scale = max(b.abs().max().item(), 1e-300)
    err = (a - b).abs().max().item()
    assert a.shape == b.shape and err <= 1e-12 * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B,H,C", [(1, 1, 8), (2, 5, 8), (3, 4, 32)])
def test_batchnorm_restatement(B, H, C, relu):
    """batchnorm_stats / batchnorm_bwd == nn.BatchNorm2d(C).train() (+ReLU) forward statistics,
    running statistics and autograd gradients; rows are the NHWC pixels."""
    g = torch.Generator().manual_seed(B * 100 + C + relu)
    bn = nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    x = (torch.randn(B, C, H, H, generator=g, dtype=F64) * 2 + 0.5).requires_grad_(True)
    dy = torch.randn(B, C, H, H, generator=g, dtype=F64)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    if B * H * H == 1:  # torch refuses one value per channel in training mode; the kernel's divisor is 1
        mean, rstd, rm, rv = E.batchnorm_stats(rows(x.detach()), bn.eps, bn.momentum, rm0, rv0, F64)
        _close(mean, rows(x.detach())[0], "mean")
        _close(rstd, torch.full((C,), bn.eps ** -0.5, dtype=F64), "rstd")
        _close(rm, 0.9 * rm0 + 0.1 * mean, "running_mean")
        _close(rv, 0.9 * rv0, "running_var")
        return
    y = bn(x)
    y = torch.relu(y) if relu else y
    y.backward(dy)
    mean, rstd, rm, rv = E.batchnorm_stats(rows(x.detach()), bn.eps, bn.momentum, rm0, rv0, F64)
    _close(rm, bn.running_mean, "running_mean")
    _close(rv, bn.running_var, "running_var")
    xd = rows(x.detach())
    _close(mean, xd.mean(0), "mean")
    _close(rstd, 1 / torch.sqrt(xd.var(0, unbiased=False) + bn.eps), "rstd")
    dx, sg, sgx = E.batchnorm_bwd(xd, rows(dy), mean, rstd, bn.weight.detach(), bn.bias.detach(), relu, F64)
    _close(dx, rows(x.grad), "dx")
    _close(sg, bn.bias.grad, "dbeta")
    _close(sgx, bn.weight.grad, "dgamma")


def test_batchnorm_mask_at_zero():
    """z == 0 is masked, as torch's relu' (0 at 0)."""
    x = torch.tensor([[1.0], [3.0]], dtype=F64)
    mean, rstd = torch.tensor([1.0], dtype=F64), torch.tensor([0.5], dtype=F64)
    one, zero = torch.ones(1, dtype=F64), torch.zeros(1, dtype=F64)
    _, sg, _ = E.batchnorm_bwd(x, torch.tensor([[7.0], [2.0]], dtype=F64), mean, rstd, one, zero, 1, F64)
    assert sg.item() == 2.0
    xz = torch.zeros(1, dtype=F64, requires_grad=True)
    torch.relu(xz).backward(torch.ones(1, dtype=F64))
    assert xz.grad.item() == 0.0


def test_bn_depth():
    """The chain lengths the GPU test's shapes rely on."""
    assert E.bn_depth(1, 8) == 1 + 256 and E.bn_depth(50, 256) == 7 + 8
    assert E.bn_depth(257, 8) == 1 + 256          # two workgroups, per = 129
    assert E.bn_depth(33025, 128) == 17 + 16      # the cap: per = 259, 16 lanes
    assert E.bn_depth(33025, 8) == 2 + 256


@pytest.mark.parametrize("B,units,D,gap", [(1, 1, 16, 0), (9, 2, 16, 8), (13, 3, 5, 0), (13, 3, 1, 4)])
def test_warp_restatement(B, units, D, gap):
    """warp_fwd / warp_bwd == the as-is Encoder4.warp (unbound: the reference's per-unit
    nn.Sequential loop) and its autograd, parameters laid out unit after unit at unit_stride."""
    from encdiff_amd.ldm.modules.diffusionmodules.openaimodel_enc import Encoder4
    torch.manual_seed(B + D)
    enc = Encoder4(8, D, units).double()
    npu = E.warp_n_per_unit(D)
    stride = npu + gap
    params = torch.full((units * stride,), float("nan"), dtype=F64)
    for i in range(units):
        flat = torch.cat([p.detach().reshape(-1) for p in enc.net[i].parameters()])
        assert flat.numel() == npu
        params[i * stride:i * stride + npu] = flat
    u = torch.randn(B, units, dtype=F64, requires_grad=True)
    out = enc.warp(u)
    _close(E.warp_fwd(u.detach(), params, stride, units, D, F64), out.detach(), "out")
    dout = torch.randn(B, units * D, dtype=F64)
    out.backward(dout)
    du, G = E.warp_bwd(u.detach(), params, stride, units, D, dout, F64)
    _close(du, u.grad, "du")
    for i in range(units):
        want = torch.cat([p.grad.reshape(-1) for p in enc.net[i].parameters()])
        _close(G[i * stride:i * stride + npu], want, f"unit {i} gradients")
        assert (G[i * stride + npu:(i + 1) * stride] == 0).all()
    s_out, s_du, s_G = E.warp_slack(u.detach(), params, stride, units, D, dout)
    assert s_out.shape == out.shape and s_du.shape == du.shape and s_G.shape == G.shape
    assert (s_out > 0).all() and (s_du >= 0).all() and torch.isfinite(s_G).all()


@pytest.mark.parametrize("B,d,units", [(1, 16, 7), (5, 24, 20), (3, 8, 64)])
def test_head_restatement(B, d, units):
    """head_fwd / head_bwd on NHWC rows == View((-1, d*16)) of the NCHW tensor + nn.Linear."""
    g = torch.Generator().manual_seed(B + d + units)
    lin = nn.Linear(d * 16, units).double()
    x = torch.randn(B, d, 4, 4, generator=g, dtype=F64, requires_grad=True)   # the trunk's NCHW output
    r = x.detach().permute(0, 2, 3, 1).reshape(B * 16, d)                     # the same as NHWC rows
    u = lin(x.view(-1, d * 16))
    _close(E.head_fwd(r, lin.weight.detach(), lin.bias.detach(), F64), u.detach(), "u")
    du = torch.randn(B, units, generator=g, dtype=F64)
    u.backward(du)
    dr, dW, db = E.head_bwd(r, lin.weight.detach(), du, F64)
    _close(dr, x.grad.permute(0, 2, 3, 1).reshape(B * 16, d), "dr")
    _close(dW, lin.weight.grad, "dW")
    _close(db, lin.bias.grad, "db")
    s = E.head_slack(r, lin.weight.detach(), lin.bias.detach(), du)
    assert [t.shape for t in s] == [u.shape, dr.shape, dW.shape, db.shape]


def test_expm1_err():
    z = torch.linspace(-20, 5, 4001, dtype=F64)
    e = E.expm1_err(z)
    assert 0 < e < 4 * 2.0 ** -23  # expm1 in (-1, 0]: a few ulps of at most 1
    assert E.expm1_err(torch.ones(3, dtype=F64)) == 0.0
