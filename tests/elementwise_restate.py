"""Pure-torch restatements of the memory-bound step kernels (csrc/elementwise.hip, the layout
kernels of csrc/bn.hip and csrc/fp32.hip), written from include/encdiff_hip.h's description of
each entry point, not from the kernels.  tests/test_gpu_elementwise.py compares the HIP kernels
with them; tests/test_elementwise_restate.py checks the restatements themselves on the CPU.

Everything here is dtype- and device-generic torch: the same function evaluated in fp64 is the
reference, evaluated in fp32 it is the "torch fp32 evaluation" whose distance from fp64 sets the
additive floors of the comparison rules below.
"""
import math

import torch

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64


# ------------------------------------------------------------------ comparison rules
def bits(t):
    """Integer view for bitwise comparisons (sentinels / -0 / NaN safe)."""
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def floor_of(t32, ref64):
    """4 x the largest |torch-fp32 evaluation - fp64| (the additive floor of both rules)."""
    if ref64.numel() == 0:
        return 0.0
    return 4.0 * (t32.double() - ref64).abs().max().item()


def bf16_excess(out, ref64, floor):
    """bf16 rule: |out - ref| <= 2^-7 |ref| + floor per element.  Returns (worst excess over the
    bound (<= 0 passes), index of the worst element, largest |out - ref|)."""
    err = (out.double() - ref64).abs()
    ex = err - (2.0 ** -7 * ref64.abs() + floor)
    i = int(ex.argmax())
    return ex.flatten()[i].item(), i, err.max().item()


def f32_excess(out, ref64, floor):
    """fp32 rule: |out - ref| <= floor + 2^-22 |ref| per element, floor = floor_of(torch fp32, ref)."""
    err = (out.double() - ref64).abs()
    ex = err - (2.0 ** -22 * ref64.abs() + floor)
    i = int(ex.argmax())
    return ex.flatten()[i].item(), i, err.max().item()


# ------------------------------------------------------------------ split-bf16
def split_bf16(w):
    """hi = bf16(w), lo = bf16(w - hi) (the subtraction is exact in fp32)."""
    w = w.to(F32)
    hi = w.to(BF16)
    lo = (w - hi.float()).to(BF16)
    return hi, lo


# ------------------------------------------------------------------ pack layouts (EncdiffPackJob)
def pack_ref(src, src_off, rows, cols, kind, cin=0):
    """The bf16 elements job (src_off, rows, cols, kind, cin) writes, flat [rows * cols]."""
    src = src.to(F32)
    n = rows * cols
    if kind == 0:  # identity
        return src[src_off:src_off + n].to(BF16)
    if kind == 1:  # conv [co][ci][3][3] -> [co][tap][ci]
        assert cols == 9 * cin
        w = src[src_off:src_off + n].view(rows, cin, 3, 3)
        return w.permute(0, 2, 3, 1).reshape(-1).to(BF16)
    if kind == 2:  # conv [co][cin][taps] -> [co][tap][8], channels cin..7 zero
        taps = cols // 8
        w = src[src_off:src_off + rows * cin * taps].view(rows, cin, taps)
        out = torch.zeros(rows, taps, 8, dtype=F32, device=src.device)
        out[:, :, :cin] = w.permute(0, 2, 1)
        return out.reshape(-1).to(BF16)
    if kind == 3:  # [co][tap][cin] -> [co][tap][hi | hi | lo]
        taps = cols // (3 * cin)
        w = src[src_off:src_off + rows * taps * cin].view(rows, taps, cin)
        hi, lo = split_bf16(w)
        return torch.cat([hi, hi, lo], dim=2).reshape(-1)
    if kind == 4:  # [co][cin][taps] (cin <= 8) -> [co][tap][hi8 | hi8 | lo8]
        taps = cols // 24
        w = src[src_off:src_off + rows * cin * taps].view(rows, cin, taps).permute(0, 2, 1)
        w8 = torch.zeros(rows, taps, 8, dtype=F32, device=src.device)
        w8[:, :, :cin] = w
        hi, lo = split_bf16(w8)
        return torch.cat([hi, hi, lo], dim=2).reshape(-1)
    if kind == 5:  # [co][cin] (co == cin) -> [co][hi | hi | lo | I | I]
        assert rows == cin and cols == 5 * cin
        w = src[src_off:src_off + rows * cin].view(rows, cin)
        hi, lo = split_bf16(w)
        eye = torch.eye(cin, dtype=BF16, device=src.device)
        return torch.cat([hi, hi, lo, eye, eye], dim=1).reshape(-1)
    if kind == 6:  # transpose: src [rows][cols] -> dst [cols][rows]
        return src[src_off:src_off + n].view(rows, cols).t().contiguous().reshape(-1).to(BF16)
    raise ValueError(kind)


def pack_src_elems(rows, cols, kind, cin=0):
    """fp32 source elements a job reads."""
    if kind in (0, 1, 6):
        return rows * cols
    if kind == 2:
        return rows * cin * (cols // 8)
    if kind == 3:
        return rows * cols // 3
    if kind == 4:
        return rows * cin * (cols // 24)
    if kind == 5:
        return rows * cin
    raise ValueError(kind)


# ------------------------------------------------------------------ layout kernels
def nchw_to_rows_ref(x, cpad, split=False):
    """fp32 NCHW [B][C][HW] -> bf16 rows [B*HW][cpad] (channels C.. zero); split: [hi | lo | hi]."""
    B, C, HW = x.shape
    r = torch.zeros(B * HW, cpad, dtype=F32, device=x.device)
    r[:, :C] = x.permute(0, 2, 1).reshape(B * HW, C)
    if not split:
        return r.to(BF16)
    hi, lo = split_bf16(r)
    return torch.cat([hi, lo, hi], dim=1)


def nchw_rows_f32_ref(x, cpad):
    """dir 0 of encdiff_nchw_rows_f32: fp32 NCHW [B][C][HW] -> rows [B*HW][cpad], padding zero."""
    B, C, HW = x.shape
    r = torch.zeros(B * HW, cpad, dtype=F32, device=x.device)
    r[:, :C] = x.permute(0, 2, 1).reshape(B * HW, C)
    return r


def rows_to_nchw_ref(rows, B, C, HW):
    """dir 1: rows [B*HW][>= C] -> NCHW [B][C][HW] (first C channels)."""
    return rows[:, :C].reshape(B, HW, C).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------ elementwise math (dtype-generic)
def silu(x):
    return x * torch.sigmoid(x)


def silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def gelu_grad(x):
    cdf = 0.5 * (1 + torch.erf(x * 0.7071067811865476))
    pdf = torch.exp(-0.5 * x * x) * 0.3989422804014327
    return cdf + x * pdf


def geglu(f):
    """f [rows][2n]: value half first, gate half second."""
    n = f.shape[1] // 2
    return f[:, :n] * gelu(f[:, n:])


def geglu_bwd(f, dy):
    n = f.shape[1] // 2
    a, g = f[:, :n], f[:, n:]
    return torch.cat([dy * gelu(g), dy * a * gelu_grad(g)], dim=1)


def _img(x, b, h, w):
    return x.reshape(b, h, w, -1)


def avgpool2(x, b, h, w):
    """rows of (b, 2h, 2w) -> rows of (b, h, w): AvgPool2d(2)."""
    s = _img(x, b, 2 * h, 2 * w)
    o = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]) * 0.25
    return o.reshape(b * h * w, -1)


def nearest2(x, b, h, w):
    """rows of (b, h/2, w/2) -> rows of (b, h, w): nearest x2."""
    s = _img(x, b, h // 2, w // 2)
    return s.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).reshape(b * h * w, -1)


def avgpool2_adjoint(dy, b, h, w):
    """dy rows of (b, h/2, w/2) -> dx rows of (b, h, w): 0.25 dy[y/2][x/2]."""
    return nearest2(dy, b, h, w) * 0.25


def nearest2_adjoint(dy, b, h, w):
    """dy rows of (b, 2h, 2w) -> dx rows of (b, h, w): the sum of the 4 children."""
    s = _img(dy, b, 2 * h, 2 * w)
    o = s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]
    return o.reshape(b * h * w, -1)


# ------------------------------------------------------------------ diffusion math
def timestep_embedding(t, dim, max_period=10000.0, dtype=F64):
    """util.py:179-199: cat[cos(t f), sin(t f)], f_k = exp(-ln(max_period) k / half)."""
    half = dim // 2
    k = torch.arange(half, dtype=dtype, device=t.device)
    freqs = torch.exp(-math.log(max_period) * k / half)
    args = t[:, None].to(dtype) * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def q_sample(x0, eps, t, sqrt_ac, sqrt_1mac, scale=None, dtype=F64):
    """x_t = sqrt_ac[t] (scale x0) + sqrt_1mac[t] eps, rows [batch][per_sample]."""
    a = sqrt_ac.to(dtype)[t][:, None]
    s = sqrt_1mac.to(dtype)[t][:, None]
    x = x0.to(dtype)
    if scale is not None:
        x = scale.to(dtype) * x
    return a * x + s * eps.to(dtype)


def ddim_step(x, e, noise, a_t, a_prev, sigma, s1, dtype=F64):
    """ddim.py:197-206 with the four coefficients given as fp32 values."""
    c = [torch.tensor(v, dtype=F32).to(dtype) for v in (a_t, a_prev, sigma, s1)]
    a_t, a_prev, sigma, s1 = c
    x, e = x.to(dtype), e.to(dtype)
    pred_x0 = (x - s1 * e) / a_t.sqrt()
    x_prev = a_prev.sqrt() * pred_x0 + (1.0 - a_prev - sigma ** 2).sqrt() * e
    if noise is not None:
        x_prev = x_prev + sigma * noise.to(dtype)
    return x_prev, pred_x0


def l1_loss(pred, eps, t, lvlb, lsw=1.0):
    """fp64 p_losses L1 (ddpm_enc.py:1194-1213): (loss, loss_vlb, loss_simple[b])."""
    ls = (pred.double() - eps.double()).abs().mean(dim=1)
    return lsw * ls.mean(), (lvlb.double()[t] * ls).mean(), ls


def l1_grad(pred, eps, lsw):
    """sign(pred - eps) * (lsw / (batch * per)) formed in fp32 as the kernel forms it: the scale is
    float(lsw) / (float(batch) * per) in fp32; exact ties give exactly 0."""
    batch, per = pred.shape
    denom = torch.tensor(float(batch), dtype=F32) * torch.tensor(float(per), dtype=F32)
    gscale = (torch.tensor(lsw, dtype=F32) / denom).to(pred.device)
    d = pred - eps
    return torch.where(d > 0, gscale, torch.where(d < 0, -gscale, torch.zeros((), device=pred.device)))


# ------------------------------------------------------------------ AdamW + EMA
def adamw_ema_step(p, g, m, v, ema, ema_n, hyper):
    """torch.optim.AdamW (single tensor: decoupled decay, lerp for exp_avg, addcmul for exp_avg_sq,
    addcdiv for the update) + LitEma (s -= (1 - decay)(s - p)) on the first ema_n elements, in the
    dtype of p.  hyper: the kernel's 8 fp32 scalars [lr, b1, b2, eps, wd, lr / bc1, 1 / sqrt(bc2),
    1 - decay] converted to that dtype (the same inputs the kernel reads).  Returns new tensors."""
    dt = p.dtype
    lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt, omd = [h.to(dt) for h in hyper.to("cpu")]
    g = g.to(dt)
    p = p * (1 - lr * wd)
    lr, b1, b2, eps, wd, step_size, inv_bc2_sqrt, omd = [float(h) for h in (lr, b1, b2, eps, wd, step_size,
                                                                            inv_bc2_sqrt, omd)]
    one_m_b1 = float(torch.tensor(1.0, dtype=dt) - torch.tensor(b1, dtype=dt))  # exact in fp32 and fp64
    one_m_b2 = float(torch.tensor(1.0, dtype=dt) - torch.tensor(b2, dtype=dt))
    m = torch.lerp(m, g, one_m_b1)
    v = (v * b2).addcmul(g, g, value=one_m_b2)
    denom = v.sqrt() * inv_bc2_sqrt + eps
    p = p - step_size * m / denom
    if ema is not None and ema_n > 0:
        ema = ema.clone()
        e = ema[:ema_n]
        ema[:ema_n] = e - omd * (e - p[:ema_n])
    return p, m, v, ema


# ------------------------------------------------------------------ gradient plumbing
def reduce_partials_ref64(part, rows, cols):
    """fp64 column sums of part[:rows, :cols] and sum |part| per column (the error scale)."""
    q = part[:rows, :cols].double()
    return q.sum(0), q.abs().sum(0)


def grad_fold_ref(gw, dw, co, cin, cpad, taps):
    """gw[o][c][t] + dw[o][t][c] (dw rows [taps][cpad]); one fp32 add per element."""
    d = dw[:co * taps * cpad].view(co, taps, cpad)[:, :, :cin].permute(0, 2, 1)
    return gw.view(co, cin, taps) + d


# ------------------------------------------------------------------ BatchNorm
def batchnorm_train(x, gamma, beta, eps, relu, dtype=F64):
    """nn.BatchNorm2d.train() over rows [N*H*W][C]: biased batch variance; returns (y, mean, rstd)."""
    x = x.to(dtype)
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * gamma.to(dtype) + beta.to(dtype)
    return (torch.relu(y) if relu else y), mean, rstd


def batchnorm_apply(x, mean, rstd, gamma, beta, relu, dtype=F64):
    y = (x.to(dtype) - mean.to(dtype)) * rstd.to(dtype) * gamma.to(dtype) + beta.to(dtype)
    return torch.relu(y) if relu else y
