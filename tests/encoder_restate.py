"""Pure-torch restatements of the concept encoder's kernels (csrc/bn.hip's training BatchNorm and
csrc/encoder.hip's warp MLPs and linear head), written from include/encdiff_hip.h's description of
each entry point and from the reference modules, not from the kernels.  tests/test_gpu_encoder.py
compares the HIP kernels with them; tests/test_encoder_restate.py checks the restatements
themselves against torch autograd on the CPU.

Every restatement takes a dtype: evaluated in fp64 it is the reference, evaluated in fp32 it is
the "torch fp32 evaluation" whose distance from fp64 sets the floor of the comparison rules
(elementwise_restate.floor_of).  The `*_slack` functions bound what the kernels' serial fp32
summation order may add on top of that floor: for a contraction of n terms added one after the
other, n * 2^-24 * sum |a_i b_i| (every partial sum is at most sum |a_i b_i| and each of the n adds
rounds it by at most 2^-24 relative), evaluated in fp64 on the reference's own intermediates and
carried to the outputs through the absolute values of the downstream weights (the pattern of
st_restate.ln_bwd_abs).
"""
import torch

F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -24  # one fp32 rounding to nearest, relative

H1, H2 = 64, 128  # the warp MLP's hidden widths
HPIX = 16         # the 4x4 grid the trunk ends on


# ------------------------------------------------------------------ BatchNorm2d.train() (+ReLU)
def batchnorm_stats(x, eps, momentum, rm, rv, dtype):
    """x [n][c] (all N*H*W pixels of a channel are rows) -> mean, rstd, running_mean, running_var.
    Biased variance under rstd, unbiased in running_var; n = 1 keeps the divisor 1."""
    x = x.to(dtype)
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    unbiased = var * (n / (n - 1 if n > 1 else 1))
    return (mean, rstd, (1 - momentum) * rm.to(dtype) + momentum * mean,
            (1 - momentum) * rv.to(dtype) + momentum * unbiased)


def batchnorm_bwd(x, dy, mean, rstd, gamma, beta, relu, dtype):
    """Backward of y = relu?(xh gamma + beta), xh = (x - mean) rstd, with the CALLER's mean / rstd.
    -> dx, sum_r g (dbeta), sum_r g xh (dgamma); g = dy where the ReLU passed (z > 0: torch's relu'
    is 0 at 0)."""
    x, dy, mean, rstd, gamma, beta = (t.to(dtype) for t in (x, dy, mean, rstd, gamma, beta))
    xh = (x - mean) * rstd
    g = torch.where(xh * gamma + beta > 0, dy, torch.zeros_like(dy)) if relu else dy
    sg, sgx = g.sum(0), (g * xh).sum(0)
    n = x.shape[0]
    dx = gamma * rstd * (g - sg / n - xh * (sgx / n))
    return dx, sg, sgx


def bn_depth(rows, c):
    """The longest fp32 addition chain of a bn.hip reduction: a workgroup (at most 128 of them, each
    a range of `per` >= 256 rows) gives each of its 256 / (c / 8) pixel lanes every lanes-th row of
    the range, then adds the lanes' sums in order; the fold across workgroups is fp64."""
    nblk = min((rows + 255) // 256, 128)
    per = (rows + nblk - 1) // nblk
    lanes = 256 // (c // 8)
    return (per + lanes - 1) // lanes + lanes


def bn_sum_slack(terms, rows, c):
    """(depth + 2) 2^-24 sum_r |term_r| per channel: `depth` adds on a term's way into its
    workgroup's partial, + 2 for the term's own product and the fp32 store of the total."""
    return (bn_depth(rows, c) + 2) * U * terms.to(F64).abs().sum(0)


def batchnorm_stats_slack(x, eps, momentum, rm, rv):
    """Bounds on |kernel - fp64| of (mean, rstd, running_mean, running_var) from the chain bound on
    S1 = sum x and S2 = sum x^2: mean = S1 / n; var = S2 / n - mean^2 moves by dS2 / n +
    2 |mean| dS1 / n; rstd = (var + eps)^-1/2 by rstd^3 / 2 per unit of var; + one fp32 rounding of
    each stored value.  running_* is (1 - m) * prior + m * new in fp32: (1 - m), both products and
    the add round once each, <= 3 x 2^-24 of the larger-magnitude sum."""
    x = x.to(F64)
    n, c = x.shape
    mean, rstd, rmn, rvn = batchnorm_stats(x, eps, momentum, rm, rv, F64)
    d1, d2 = bn_sum_slack(x, n, c), bn_sum_slack(x * x, n, c)
    dmean = d1 / n
    dvar = d2 / n + 2 * mean.abs() * d1 / n
    s_mean = dmean + U * mean.abs()
    s_rstd = 0.5 * rstd ** 3 * dvar + U * rstd
    nb = n / (n - 1 if n > 1 else 1)
    var = ((x - mean) ** 2).mean(0)
    s_rm = momentum * s_mean + 3 * U * ((1 - momentum) * rm.to(F64).abs() + momentum * mean.abs())
    s_rv = momentum * nb * (dvar + U * var) + 3 * U * ((1 - momentum) * rv.to(F64).abs() + momentum * nb * var)
    return s_mean, s_rstd, s_rm, s_rv


# ------------------------------------------------------------------ Encoder4.warp
def warp_n_per_unit(D):
    return 2 * H1 + H2 * H1 + H2 + D * H2 + D


def _unit_params(params, unit_stride, units, D, dtype):
    """[W1 64][b1 64][W2 128x64][b2 128][W3 D x 128][b3 D] of each unit at unit_stride"""
    P = torch.as_strided(params.to(dtype), (units, warp_n_per_unit(D)), (unit_stride, 1))
    o = [0, H1, 2 * H1, 2 * H1 + H2 * H1, 2 * H1 + H2 * H1 + H2, 2 * H1 + H2 * H1 + H2 + D * H2]
    return (P[:, o[0]:o[1]], P[:, o[1]:o[2]], P[:, o[2]:o[3]].reshape(units, H2, H1), P[:, o[3]:o[4]],
            P[:, o[4]:o[5]].reshape(units, D, H2), P[:, o[5]:])


def _elu(z):
    return torch.where(z > 0, z, torch.expm1(z))


def _elu_d(out):
    """ELU' from the OUTPUT (torch's elu_backward with is_result): out > 0 ? 1 : out + 1"""
    return torch.where(out > 0, torch.ones_like(out), out + 1)


def warp_hidden(u, params, unit_stride, units, D, dtype):
    """-> (z1, h1, z2, h2), each [units][B][width]"""
    W1, b1, W2, b2, _, _ = _unit_params(params, unit_stride, units, D, dtype)
    ut = u.to(dtype).t()[:, :, None]                               # [U][B][1]
    z1 = ut * W1[:, None, :] + b1[:, None, :]
    h1 = _elu(z1)
    z2 = torch.einsum("ubj,ukj->ubk", h1, W2) + b2[:, None, :]
    return z1, h1, z2, _elu(z2)


def warp_fwd(u, params, unit_stride, units, D, dtype):
    """u [B][units] -> out [B][units * D]: Linear(1,64) -> ELU -> Linear(64,128) -> ELU -> Linear(128,D)"""
    _, _, _, _, W3, b3 = _unit_params(params, unit_stride, units, D, dtype)
    h2 = warp_hidden(u, params, unit_stride, units, D, dtype)[3]
    o = torch.einsum("ubk,umk->ubm", h2, W3) + b3[:, None, :]
    return o.permute(1, 0, 2).reshape(u.shape[0], units * D)


def _warp_pack(units, unit_stride, D, dW1, db1, dW2, db2, dW3, db3):
    G = torch.zeros(units, unit_stride, dtype=dW1.dtype, device=dW1.device)
    G[:, :warp_n_per_unit(D)] = torch.cat([dW1, db1, dW2.reshape(units, -1), db2, dW3.reshape(units, -1), db3], 1)
    return G.reshape(-1)


def warp_bwd(u, params, unit_stride, units, D, dout, dtype):
    """-> du [B][units], and the parameter gradients in the parameters' own block layout
    [units * unit_stride] (zero in the gaps)."""
    W1, _, W2, _, W3, _ = _unit_params(params, unit_stride, units, D, dtype)
    _, h1, _, h2 = warp_hidden(u, params, unit_stride, units, D, dtype)
    B = u.shape[0]
    do = dout.to(dtype).reshape(B, units, D).permute(1, 0, 2)      # [U][B][D]
    ut = u.to(dtype).t()[:, :, None]
    dW3 = torch.einsum("ubm,ubk->umk", do, h2)
    dz2 = torch.einsum("ubm,umk->ubk", do, W3) * _elu_d(h2)
    dW2 = torch.einsum("ubk,ubj->ukj", dz2, h1)
    dz1 = torch.einsum("ubk,ukj->ubj", dz2, W2) * _elu_d(h1)
    du = (dz1 * W1[:, None, :]).sum(2).t()
    return du, _warp_pack(units, unit_stride, D, (dz1 * ut).sum(1), dz1.sum(1), dW2, dz2.sum(1), dW3, do.sum(1))


def expm1_err(z):
    """4 x the largest |torch.expm1 in fp32 - fp64| over the negative entries of z (fp64): the
    allowance for the kernels' expm1f"""
    z = z[z <= 0]
    if z.numel() == 0:
        return 0.0
    z32 = z.to(F32)
    return 4.0 * (torch.expm1(z32).double() - torch.expm1(z32.double())).abs().max().item()


def warp_slack(u, params, unit_stride, units, D, dout):
    """Bounds on what the kernels' serial fp32 order may add to the floor, per element of
    (out, du, grads): every contraction on the output's path contributes n 2^-24 sum |a_i b_i| (n its
    number of serial adds), earlier stages' bounds are carried on through |downstream weight| and
    |ELU'| <= 1, and each ELU on the negative side adds expm1_err.  The batch contractions of the
    parameter gradients are min(B, 8) adds inside a chunk, then ceil(B / 8) chunk partials added in
    order, then the add into `grads`."""
    W1, b1, W2, b2, W3, b3 = (t.abs() for t in _unit_params(params, unit_stride, units, D, F64))
    z1, h1, z2, h2 = warp_hidden(u, params, unit_stride, units, D, F64)
    B = u.shape[0]
    ut = u.to(F64).t()[:, :, None].abs()
    ex = max(expm1_err(z1), expm1_err(z2))
    neg1, neg2 = (z1 <= 0).double(), (z2 <= 0).double()
    e_z1 = 2 * U * (ut * W1[:, None, :] + b1[:, None, :])
    e_h1 = e_z1 + ex * neg1
    a1 = h1.abs()
    e_z2 = (H1 + 1) * U * (torch.einsum("ubj,ukj->ubk", a1, W2) + b2[:, None, :]) + torch.einsum("ubj,ukj->ubk", e_h1, W2)
    e_h2 = e_z2 + ex * neg2
    a2 = h2.abs()
    s_out = (H2 + 1) * U * (torch.einsum("ubk,umk->ubm", a2, W3) + b3[:, None, :]) + torch.einsum("ubk,umk->ubm", e_h2, W3)
    s_out = s_out.permute(1, 0, 2).reshape(B, units * D)

    nb = min(B, 8) + (B + 7) // 8 + 1
    P = _unit_params(params, unit_stride, units, D, F64)
    do = dout.to(F64).reshape(B, units, D).permute(1, 0, 2)
    ado = do.abs()
    s_dW3 = nb * U * torch.einsum("ubm,ubk->umk", ado, a2) + torch.einsum("ubm,ubk->umk", ado, e_h2)
    s_db3 = nb * U * ado.sum(1)
    dh2 = torch.einsum("ubm,umk->ubk", do, P[4])
    d2 = _elu_d(h2)
    dz2 = dh2 * d2
    # dz2 = dh2 * ELU'(h2): the contraction over D, ELU' = h2 + 1 (its error e_h2 + one rounding), the product
    e_dz2 = D * U * torch.einsum("ubm,umk->ubk", ado, W3) * d2 + dh2.abs() * (e_h2 + U) * neg2 + U * dz2.abs()
    adz2 = dz2.abs()
    s_dW2 = (nb * U * torch.einsum("ubk,ubj->ukj", adz2, a1) + torch.einsum("ubk,ubj->ukj", e_dz2, a1)
             + torch.einsum("ubk,ubj->ukj", adz2, e_h1))
    s_db2 = nb * U * adz2.sum(1) + e_dz2.sum(1)
    dh1 = torch.einsum("ubk,ukj->ubj", dz2, P[2])
    d1 = _elu_d(h1)
    dz1 = dh1 * d1
    e_dz1 = ((H2 * U * torch.einsum("ubk,ukj->ubj", adz2, W2) + torch.einsum("ubk,ukj->ubj", e_dz2, W2)) * d1
             + dh1.abs() * (e_h1 + U) * neg1 + U * dz1.abs())
    adz1 = dz1.abs()
    s_dW1 = (nb + 1) * U * (adz1 * ut).sum(1) + (e_dz1 * ut).sum(1)
    s_db1 = nb * U * adz1.sum(1) + e_dz1.sum(1)
    s_du = ((H1 + 1) * U * (adz1 * W1[:, None, :]).sum(2) + (e_dz1 * W1[:, None, :]).sum(2)).t()
    return s_out, s_du, _warp_pack(units, unit_stride, D, s_dW1, s_db1, s_dW2, s_db2, s_dW3, s_db3)


# ------------------------------------------------------------------ View + Linear head
def head_flat(r, d, dtype):
    """NHWC rows r[(b*16 + p)][c] -> the reference's flatten [B][k = c*16 + p]"""
    B = r.shape[0] // HPIX
    return r.to(dtype).reshape(B, HPIX, d).permute(0, 2, 1).reshape(B, d * HPIX)


def head_fwd(r, W, bias, dtype):
    """u = View((-1, d*16))(NCHW trunk output) @ W^T + bias, W [units][d*16]"""
    return head_flat(r, W.shape[1] // HPIX, dtype) @ W.to(dtype).t() + bias.to(dtype)


def head_bwd(r, W, du, dtype):
    """-> dr (NHWC rows like r), dW, db"""
    d = W.shape[1] // HPIX
    B = du.shape[0]
    du = du.to(dtype)
    dr = (du @ W.to(dtype)).reshape(B, d, HPIX).permute(0, 2, 1).reshape(B * HPIX, d)
    return dr, du.t() @ head_flat(r, d, dtype), du.sum(0)


def head_slack(r, W, bias, du):
    """Serial-order bounds for (u, dr, dW, db).  u: a lane adds ceil(K / 64) products, the wave sum
    is 6 butterfly adds, + the bias.  dr: `units` products in order.  dW: an image group adds
    ceil(B / 16) products, then the 16 groups in order, then the add into dW.  db: ceil(B / 4)
    then 4 groups, then the add."""
    d = W.shape[1] // HPIX
    K, B, units = W.shape[1], du.shape[0], W.shape[0]
    af, aW, adu = head_flat(r, d, F64).abs(), W.to(F64).abs(), du.to(F64).abs()
    s_u = ((K + 63) // 64 + 6 + 1) * U * (af @ aW.t() + bias.to(F64).abs())
    s_dr = units * U * (adu @ aW).reshape(B, d, HPIX).permute(0, 2, 1).reshape(B * HPIX, d)
    s_dW = ((B + 15) // 16 + 16 + 1) * U * (adu.t() @ af)
    s_db = ((B + 3) // 4 + 4 + 1) * U * adu.sum(0)
    return s_u, s_dr, s_dW, s_db
