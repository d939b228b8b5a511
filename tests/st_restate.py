"""Pure-torch restatement of the fused SpatialTransformer kernels (csrc/st_fused.hip, csrc/st_bwd.hip),
written from include/encdiff_hip.h (EncdiffStTailArgs, EncdiffStHeadArgs, EncdiffStTailBwdArgs,
EncdiffStHeadBwdArgs) and the block they fuse (ldm/modules/attention.py: SpatialTransformer,
BasicTransformerBlock, CrossAttention, GEGLU), one function per stage, and a Python copy of the four
entry points' dispatch (StPlan).  tests/test_gpu_st.py compares the HIP kernels with it stage by
stage; tests/test_st_restate.py checks it on the CPU against the block's fp64 arithmetic and torch
autograd, and pins the dispatch table.

Every stage function takes the stage's inputs (any dtype: they are converted to `dt`) and returns its
output in `dt`: evaluated in fp64 it is the reference, in fp32 the "torch fp32 evaluation" whose
distance from fp64 sets the additive floor (elementwise_restate.floor_of).  Weights are [out][in]
(nn.Linear); rows are [B * tokens][c]; the concept tokens' K / V rows are [B * n_ctx][c].

ST_ROUNDS says, per stage, what the kernels round to bf16 and what stays fp32 (read off the kernels;
the arithmetic itself is restated from the header and attention.py).
"""
import os
from types import SimpleNamespace

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
OK, ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -3
HEADS = 8
KNOBS = ("ENCDIFF_ST_BWD_MF", "ENCDIFF_ST_TAIL_STATS_ADD", "ENCDIFF_ST_TAIL_R32_C64")
LDS_MAX = 160 * 1024

ST_ROUNDS = {
    # forward head (st_head_kernel)
    "gn_stats": "fp32 (mean, rstd) from fp32 sums: var = E[x^2] - mean^2 clamped at 0",
    "gn": "x * (rstd gamma) + (beta - mean rstd gamma) in fp32, rounded once (MFMA operand; stored when gn is given)",
    "t0": "fp32 accumulation + bias; rounded once when stored; LN1 reads the ROUNDED row",
    "s1": "fp32 statistics of the bf16-rounded t0 row (two-pass variance)",
    "n1": "rounded once (MFMA operand; stored in training)",
    "qkv": "fp32 accumulation, rounded once",
    # forward tail (st_tail_kernel)
    "t1": "o1 Wout1^T + b + t0 in fp32: the residual stream Tr is NEVER rounded; save_t1 = bf16(Tr)",
    "s2": "fp32 statistics of bf16(t1) (the saved row)",
    "n2": "LN of bf16(t1), rounded once (operand and save)",
    "q2": "rounded once (operand of the cross-attention and save)",
    "o2": "scores, softmax and p v in fp32 from the bf16 q2 / k2 / v2 (exp: fast exp2 form); rounded once",
    "lse2": "fp32: max + log(sum), natural log",
    "t2": "o2 Wout2^T + b + Tr (the UNROUNDED t1) in fp32; save_t2 / head_t2 = bf16(Tr)",
    "s3": "fp32 statistics of bf16(t2)",
    "n3": "LN of bf16(t2), rounded once",
    "f": "n3 W1^T + b in fp32, rounded once; a is formed from the ROUNDED f",
    "a": "v * gelu(g) on the rounded f (erf by Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7), rounded once",
    "t3": "a W2^T + b + Tr (the UNROUNDED t2) in fp32; rounded once: the operand of proj_out IS save_t3",
    "out": "bf16(t3) Wpo^T + b + x in fp32, rounded once",
    "slots": "fp32 sum and sum of squares of the STORED bf16 out per 64-row segment and column",
    # backward tail (st_tail_bwd_kernel)
    "d_t3": "dy Wpo in fp32: the residual-gradient stream Tr (never rounded); stored / operand = bf16(Tr)",
    "d_a": "bf16(d_t3) W2, ROUNDED to bf16 before the GEGLU backward (not stored)",
    "d_f": "(d_a gelu(g), d_a v gelu'(g)) in fp32 from the rounded d_a and the saved f; rounded once (stored = operand)",
    "d_n3": "d_f W1 in fp32, ROUNDED to bf16 (not stored)",
    "d_t2": "Tr += LN3'(saved t2, s3; d_n3): fp32; stored / operand = bf16(Tr)",
    "ln_part": "fp32 sums over the tile's rows of d xh and of d (d the ROUNDED d_n3 / d_n2 / d_n1)",
    "d_o2": "bf16(d_t2) Wout2, ROUNDED to bf16 (not stored)",
    "d_q2": "D, p = exp(s - lse2), dS, dq in fp32 from bf16 q2 k2 v2 o2 d_o2; rounded once (stored = operand)",
    "dkv": "MF form: P and dS ROUNDED to bf16, dV = P^T dO, dK = scale dS^T Q on MFMA (fp32 accumulation); "
           "VALU form: everything fp32.  One tile per image: rounded once into dk2 / dv2; several: fp32 slabs",
    "d_n2": "d_q2 Wq2, ROUNDED to bf16 (not stored)",
    "d_t1": "Tr += LN2'(saved t1, s2; d_n2); stored / operand = bf16(Tr)",
    "d_o1": "bf16(d_t1) Wout1, rounded once",
    # backward head (st_head_bwd_kernel)
    "kv_fold": "in-order fp32 sum of an image's slabs, rounded once (exact restatement)",
    "d_n1": "d_qkv Wqkv, ROUNDED to bf16 (not stored)",
    "d_t0": "d_t1 (bf16 input, exact in fp32) + LN1'(saved t0, s1; d_n1); rounded once (stored = operand)",
    "d_gn": "bf16(d_t0) Win, rounded once",
}


def rb(t, on=True):
    """One bf16 rounding (round to nearest even), kept in t's dtype."""
    return t.to(BF16).to(t.dtype) if on else t


# ------------------------------------------------------------------ stages: linear / norms
def lin(x, W, b=None, res=None, dt=F64):
    """y = x W^T (+ b) (+ res)"""
    y = x.to(dt) @ W.to(dt).t()
    if b is not None:
        y = y + b.to(dt)
    if res is not None:
        y = y + res.to(dt)
    return y


def lin_bwd(dy, W, dt=F64):
    """input gradient of y = x W^T: dx = dy W"""
    return dy.to(dt) @ W.to(dt)


def ln_stats(x, eps, dt=F64):
    """(mean, rstd) [rows][2] of nn.LayerNorm (biased variance)"""
    x = x.to(dt)
    m = x.mean(1, keepdim=True)
    v = ((x - m) ** 2).mean(1, keepdim=True)
    return torch.cat([m, torch.rsqrt(v + eps)], 1)


def ln_apply(x, st, g, b, dt=F64):
    st = st.to(dt)
    return (x.to(dt) - st[:, :1]) * st[:, 1:] * g.to(dt) + b.to(dt)


def ln_bwd(x, st, g, d, dt=F64):
    """dx of y = LN(x) g + b for dy = d from the saved (mean, rstd): xh = (x - mean) rstd, gd = d g,
    dx = rstd (gd - mean_c(gd) - xh mean_c(gd xh))."""
    st = st.to(dt)
    xh = (x.to(dt) - st[:, :1]) * st[:, 1:]
    gd = d.to(dt) * g.to(dt)
    return st[:, 1:] * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))


def ln_bwd_abs(x, st, g, h):
    """What an error of magnitude h in d moves ln_bwd's dx by, at most (fp64): the same contraction
    with absolute values."""
    st = st.to(F64)
    xh = ((x.to(F64) - st[:, :1]) * st[:, 1:]).abs()
    gh = h.to(F64) * g.to(F64).abs()
    return st[:, 1:].abs() * (gh + gh.mean(1, keepdim=True) + xh * (gh * xh).mean(1, keepdim=True))


def ln_partials(x, st, d, tile, dt=F64):
    """per tile of `tile` rows: (sum_r d xh, sum_r d), each [rows / tile][c]"""
    st = st.to(dt)
    xh = (x.to(dt) - st[:, :1]) * st[:, 1:]
    d = d.to(dt)
    c = d.shape[1]
    return (d * xh).reshape(-1, tile, c).sum(1), d.reshape(-1, tile, c).sum(1)


def ln_partials_abs(x, st, h, tile):
    st = st.to(F64)
    xh = ((x.to(F64) - st[:, :1]) * st[:, 1:]).abs()
    h = h.to(F64)
    c = h.shape[1]
    return (h * xh).reshape(-1, tile, c).sum(1), h.reshape(-1, tile, c).sum(1)


def gn_sums(x, dt=F64):
    """The producer statistics of rows x (EncdiffGemmArgs.gn_stats layout): per 64-row segment two
    rows, the per-column sum and sum of squares -> [2 * rows / 64][c]."""
    x = x.to(dt).reshape(-1, 64, x.shape[1])
    return torch.stack([x.sum(1), (x * x).sum(1)], 1).reshape(-1, x.shape[2])


def gn_stats_from_sums(sums, B, tokens, c, eps, dt=F64):
    """(mean, rstd) [B][32][2] of GroupNorm32 from the segment sums (tokens % 64 == 0)."""
    s = sums.to(dt)[:, :c].reshape(B, tokens // 64, 2, 32, c // 32).sum((1, 4))  # [B][2][32]
    n = tokens * (c // 32)
    mean = s[:, 0] / n
    var = (s[:, 1] / n - mean * mean).clamp_min(0)
    return torch.stack([mean, torch.rsqrt(var + eps)], 2)


def gn_stats_from_x(x, B, tokens, c, eps, dt=F64):
    x = x.to(dt).reshape(B, tokens, 32, c // 32)
    n = tokens * (c // 32)
    mean = x.sum((1, 3)) / n
    var = ((x * x).sum((1, 3)) / n - mean * mean).clamp_min(0)
    return torch.stack([mean, torch.rsqrt(var + eps)], 2)


def gn_apply(x, st, gamma, beta, B, tokens, dt=F64):
    """GroupNorm32 apply from (mean, rstd) [B][32][2]"""
    c = x.shape[1]
    st = st.to(dt).reshape(B, 1, 32, 1, 2)
    x = x.to(dt).reshape(B, tokens, 32, c // 32)
    a = st[..., 1] * gamma.to(dt).reshape(1, 1, 32, c // 32)
    return (x * a + (beta.to(dt).reshape(1, 1, 32, c // 32) - st[..., 0] * a)).reshape(B * tokens, c)


# ------------------------------------------------------------------ stages: cross-attention to the concept tokens
def _heads(t, B, S):
    """rows [B * S][c] -> [B][8][S][dh]"""
    return t.reshape(B, S, HEADS, t.shape[1] // HEADS).permute(0, 2, 1, 3)


def _rows(t):
    """[B][8][S][dh] -> rows"""
    B, H, S, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * dh)


def cross_attn(q2, k2, v2, B, tokens, nctx, dt=F64):
    """o2 = softmax(q2 k2^T dh^-0.5) v2 per (image, head); lse2 [B * 8][tokens] (natural log).
    Also abs_o = P |v| and xmax = max |s - lse| (what a relative error of exp scales with)."""
    q, k, v = _heads(q2.to(dt), B, tokens), _heads(k2.to(dt), B, nctx), _heads(v2.to(dt), B, nctx)
    s = q @ k.transpose(2, 3) * (q.shape[3] ** -0.5)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    return SimpleNamespace(o=_rows(P @ v), lse=lse.reshape(B * HEADS, tokens), abs_o=_rows(P @ v.abs()),
                           xmax=(s - lse[..., None]).abs().max().item())


def cross_attn_bwd(q2, k2, v2, o2, lse2, d_o2, B, tokens, nctx, tile, dt=F64, h_do=None, mf=False, exp_rel=0.0):
    """From its givens (attention.py:180-191 differentiated, the softmax recomputed from the saved
    LSE): P = exp(s - lse2), D = rowsum(d_o2 o2), dS = P (d_o2 v^T - D), dq = dS k scale, and per
    tile of `tile` rows dK = scale dS^T q, dV = P^T d_o2 -> dq rows and dkv [rows / tile][n_ctx][2c]
    (dK | dV: the kv_part slab layout; tile == tokens: the rows of dk2 | dv2).
    h_do (fp64 only): the error magnitude of d_o2 per element; then .s_dq / .s_dkv bound what it, a
    relative error exp_rel of every p and (mf) the bf16 roundings of P and dS move the results by."""
    q, k, v = _heads(q2.to(dt), B, tokens), _heads(k2.to(dt), B, nctx), _heads(v2.to(dt), B, nctx)
    o, do = _heads(o2.to(dt), B, tokens), _heads(d_o2.to(dt), B, tokens)
    dh = q.shape[3]
    scale = dh ** -0.5
    s = q @ k.transpose(2, 3) * scale
    P = torch.exp(s - lse2.to(dt).reshape(B, HEADS, tokens, 1))
    D = (do * o).sum(-1, keepdim=True)
    dS = P * (do @ v.transpose(2, 3) - D)
    tpi = tokens // tile

    def per_tile(a, b):  # a [B][8][tokens][n_ctx], b [B][8][tokens][dh] -> [B][tpi][n_ctx][8 dh]
        a = a.reshape(B, HEADS, tpi, tile, nctx).transpose(3, 4)
        b = b.reshape(B, HEADS, tpi, tile, dh)
        return (a @ b).permute(0, 2, 3, 1, 4).reshape(B, tpi, nctx, HEADS * dh)

    def slabs(dk, dv):
        return torch.cat([dk, dv], 3).reshape(B * tpi, nctx, 2 * HEADS * dh)

    r = SimpleNamespace(dq=_rows(dS @ k * scale), dkv=slabs(per_tile(dS, q) * scale, per_tile(P, do)))
    if h_do is not None:
        h = _heads(h_do.to(dt), B, tokens)
        # |error of dS| <= P (h |v|^T + h . |o|) + 2 exp_rel |dS|-like terms
        e_ds = P * (h @ v.abs().transpose(2, 3) + (h * o.abs()).sum(-1, keepdim=True)) + \
            exp_rel * P * (do.abs() @ v.abs().transpose(2, 3) + (do.abs() * o.abs()).sum(-1, keepdim=True))
        e_p = exp_rel * P
        r.s_dq = _rows(e_ds @ k.abs() * scale)
        if mf:  # P and dS rounded to bf16 before the key-gradient MFMAs
            e_p = e_p + half_ulp(P + e_p)
            e_ds = e_ds + half_ulp(dS.abs() + e_ds)
        r.s_dkv = slabs(per_tile(e_ds, q.abs()) * scale, per_tile(e_p, do.abs()) + per_tile(P, h))
    return r


# ------------------------------------------------------------------ stages: GEGLU
def gelu(x):
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def geglu(f, dt=F64):
    """a = f_v gelu(f_g): value columns first, gate columns second (attention.py:37-44)"""
    f = f.to(dt)
    n = f.shape[1] // 2
    return f[:, :n] * gelu(f[:, n:])


def geglu_bwd(f, d_a, dt=F64):
    """d_f = (d_a gelu(g) | d_a v gelu'(g))"""
    f, d_a = f.to(dt), d_a.to(dt)
    n = f.shape[1] // 2
    return torch.cat([d_a * gelu(f[:, n:]), d_a * f[:, :n] * gelu_grad(f[:, n:])], 1)


# ------------------------------------------------------------------ chains (rounding on: the kernels' roundings)
def head_fwd(x, P, B, tokens, gn_eps=1e-6, ln_eps=1e-5, rounds=True, dt=F64):
    """gn = GroupNorm32(x), t0 = proj_in(gn), n1 = LN1(t0), qkv = n1 [Wq; Wk; Wv]^T"""
    c = x.shape[1]
    r = SimpleNamespace()
    r.gn_stats = gn_stats_from_x(x, B, tokens, c, gn_eps, dt)
    r.gn = rb(gn_apply(x, r.gn_stats, P["gn_g"], P["gn_b"], B, tokens, dt), rounds)
    r.t0 = rb(lin(r.gn, P["in"], P["b_in"], dt=dt), rounds)
    r.s1 = ln_stats(r.t0, ln_eps, dt)
    r.n1 = rb(ln_apply(r.t0, r.s1, P["g1"], P["be1"], dt), rounds)
    r.qkv = rb(lin(r.n1, P["qkv"], dt=dt), rounds)
    return r


def tail_fwd(o1, t0, x, k2, v2, P, B, tokens, nctx, ln_eps=1e-5, rounds=True, dt=F64):
    """The chain of encdiff_st_tail_fwd with the kernel's roundings (rounds) or none."""
    r = SimpleNamespace()
    tr = lin(o1, P["out1"], P["b_out1"], t0, dt)          # the fp32 residual stream: not rounded
    r.t1 = rb(tr, rounds)
    r.s2 = ln_stats(r.t1, ln_eps, dt)
    r.n2 = rb(ln_apply(r.t1, r.s2, P["g2"], P["be2"], dt), rounds)
    r.q2 = rb(lin(r.n2, P["q2"], dt=dt), rounds)
    at = cross_attn(r.q2, k2, v2, B, tokens, nctx, dt)
    r.o2, r.lse2 = rb(at.o, rounds), at.lse
    tr = lin(r.o2, P["out2"], P["b_out2"], tr, dt)
    r.t2 = rb(tr, rounds)
    r.s3 = ln_stats(r.t2, ln_eps, dt)
    r.n3 = rb(ln_apply(r.t2, r.s3, P["g3"], P["be3"], dt), rounds)
    r.f = rb(lin(r.n3, P["ff1"], P["b_ff1"], dt=dt), rounds)
    r.a = rb(geglu(r.f, dt), rounds)
    r.t3 = rb(lin(r.a, P["ff2"], P["b_ff2"], tr, dt), rounds)
    r.out = rb(lin(r.t3, P["po"], P["b_po"], x, dt), rounds)
    return r


def tail_bwd(dy, sv, k2, v2, P, B, tokens, nctx, tile, rounds=True, dt=F64):
    """The chain of encdiff_st_tail_bwd from the forward's saves sv (f t2 t1 q2 o2 s3 s2 lse2)."""
    r = SimpleNamespace()
    tr = lin_bwd(dy, P["po"], dt)
    r.d_t3 = rb(tr, rounds)
    d_a = rb(lin_bwd(r.d_t3, P["ff2"], dt), rounds)
    r.d_f = rb(geglu_bwd(sv.f, d_a, dt), rounds)
    d_n3 = rb(lin_bwd(r.d_f, P["ff1"], dt), rounds)
    r.ln3 = ln_partials(sv.t2, sv.s3, d_n3, tile, dt)
    tr = tr + ln_bwd(sv.t2, sv.s3, P["g3"], d_n3, dt)
    r.d_t2 = rb(tr, rounds)
    d_o2 = rb(lin_bwd(r.d_t2, P["out2"], dt), rounds)
    at = cross_attn_bwd(sv.q2, k2, v2, sv.o2, sv.lse2, d_o2, B, tokens, nctx, tile, dt)
    r.d_q2, r.dkv = rb(at.dq, rounds), at.dkv
    d_n2 = rb(lin_bwd(r.d_q2, P["q2"], dt), rounds)
    r.ln2 = ln_partials(sv.t1, sv.s2, d_n2, tile, dt)
    tr = tr + ln_bwd(sv.t1, sv.s2, P["g2"], d_n2, dt)
    r.d_t1 = rb(tr, rounds)
    r.d_o1 = rb(lin_bwd(r.d_t1, P["out1"], dt), rounds)
    return r


def head_bwd(d_qkv, d_t1, t0, s1, P, tile, rounds=True, dt=F64):
    r = SimpleNamespace()
    d_n1 = rb(lin_bwd(d_qkv, P["qkv"], dt), rounds)
    r.ln1 = ln_partials(t0, s1, d_n1, tile, dt)
    r.d_t0 = rb(d_t1.to(dt) + ln_bwd(t0, s1, P["g1"], d_n1, dt), rounds)
    r.d_gn = rb(lin_bwd(r.d_t0, P["in"], dt), rounds)
    return r


def kv_fold(kv_part, tpi):
    """The head backward's fold: an image's slabs summed in tile order in fp32, rounded once.
    kv_part fp32 [B * tpi][n_ctx][2c] -> bf16 [B * n_ctx][2c] (dK | dV).  Exact."""
    s = kv_part.reshape(-1, tpi, kv_part.shape[1], kv_part.shape[2]).to(F32)
    a = s[:, 0].clone()
    for z in range(1, tpi):
        a = a + s[:, z]
    return a.reshape(-1, kv_part.shape[2]).to(BF16)


# ------------------------------------------------------------------ bound helpers
# A bf16 value keeps 8 significant bits, so ONE rounding to nearest of v moves it by at most half a
# unit in the last place of v's binade, 2^(floor(log2 |v|) - 8): between 2^-9 |v| (v just below a
# power of two) and 2^-8 |v| (v a power of two).  The helpers use that exact half-ulp, not a
# relative constant: 2^-9 |v| alone is the figure a sum of many roundings averages to, and a
# correctly rounded single store exceeds it for about a quarter of all values (test_half_ulp).
#   * a stored bf16 output whose fp32 value is within s of the reference:  s + half_ulp(|ref| + s)
#   * an operand the kernel rounds that is NOT stored (d_a, d_n3, d_o2, d_n2, d_n1, the gn / n1 of the
#     forms that do not write them): the reference keeps it unrounded and the consumer's contraction
#     is repeated on half_ulp(|operand| + floor) with absolute values (|W|, ln_bwd_abs, ...)
#   * the fp32 residual stream a stage reads unrounded while only its bf16 rounding is stored (t1 in
#     t2, t2 in t3, d_t3 in d_t2, d_t2 in d_t1): half_ulp(|saved value|)
#   * fp32 outputs: the fp32 rule, slack + floor + 2^-22 |ref|
#   * the floor: elementwise_restate.floor_of, 4 x |fp32 evaluation - fp64| of the same restatement
def half_ulp(v):
    """Half a bf16 ulp of |v| (fp64 tensor): 2^(floor(log2 |v|) - 8); 0 for 0.  Subnormals: 2^-134."""
    v = v.abs().double()
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -126)))
    return torch.where(v > 0, torch.exp2(e - 8), torch.zeros_like(v))


def bf16_store_tol(ref64, s):
    """|stored bf16 - ref| allowed when the kernel's fp32 value is within s of ref (s: tensor or float)"""
    s = torch.as_tensor(s, dtype=F64, device=ref64.device)
    return s + half_ulp(ref64.abs() + s)


def f32_tol(ref64, s):
    return torch.as_tensor(s, dtype=F64, device=ref64.device) + 2.0 ** -22 * ref64.abs()


# gelu_fast / gelu_and_grad: erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7 in exact arithmetic)
# evaluated in fp32: a reciprocal and an exp of 1 ulp each and a five-term Horner form whose
# intermediates stay below 1.5 -- eight roundings of at most 1.5 * 2^-24 -- so
ERF_ERR = 1.5e-7 + 8 * 1.5 * 2.0 ** -24


def gelu_slack(g):
    """|gelu_fast(g) - gelu(g)| <= |g| / 2 * ERF_ERR"""
    return 0.5 * g.abs().double() * ERF_ERR


def gelu_grad_slack(g):
    """gelu' = cdf + g pdf: the cdf carries ERF_ERR / 2, the density term the fast exp's relative
    error (exp_rel_of(g^2 / 2)) of |g| pdf <= 0.25"""
    g = g.abs().double()
    return 0.5 * ERF_ERR + g * torch.exp(-0.5 * g * g) * 0.3989422804014327 * (2.0 ** -23 * (2 + 0.5 * g * g))


def exp_rel_of(xmax):
    """Relative error of the kernels' fast exp (exp2(x log2 e) on v_exp_f32, 1 ulp) for |x| <= xmax:
    the product's rounding moves the exponent by 2^-24 |x| log2 e, i.e. the result by 2^-24 |x|
    relative, + 2^-23 for the instruction and the final rounding."""
    return 2.0 ** -23 * (2 + xmax)


# ------------------------------------------------------------------ dispatch (a copy of the four entry points')
def tail_fwd_lds(c, R, nimg, nctx):
    return R * (c + 4) * 4 + 2 * R * (c + 8) * 2 + nimg * 2 * nctx * c * 2


def head_fwd_lds(c, R, nimg, nwv, self_stats):
    return R * (c + 4) * 4 + R * (c + 8) * 2 + R * (3 * c + 8) * 2 + nimg * 64 * 4 + (64 * 64 * nwv if self_stats else 0)


def tail_bwd_lds(c, R, nctx, mf):
    """TailBwd<C, R>::lds_bytes"""
    ldt, ldx, ldh = c + 4, c + 8, 2 * 64 + 8
    ub = (max(R * ldh * 2, R * ldt * 4, R * ldx * 2) + 15) // 16 * 16
    qb = R * ldx * 2
    ps = 256 * ((nctx + 3) & ~3) * 2 * 2 + 64
    u = max(ub, qb + ps) if mf else ub + 2 * R * 8 * 4
    return R * ldt * 4 + 2 * R * ldx * 2 + 2 * nctx * c * 2 + u + 16


def tail_bwd_mf(c, R, nctx):
    """The MFMA key-gradient form where its P / dS round fits the occupancy the tile was sized for"""
    cap = 160 * 1024 if (c == 128 and R == 64) else 80 * 1024
    return tail_bwd_lds(c, R, nctx, True) <= cap


def mf_last(c, R):
    """The largest n_ctx that still takes the MF form"""
    return max(n for n in range(1, 65) if tail_bwd_mf(c, R, n))


class StPlan:
    """What the four entry points do with a shape at the default knobs: .rc (OK / ERR_SHAPE /
    ERR_UNSUPPORTED; ERR_ARG conditions on pointers are not modelled), and when OK .tile (rows per
    workgroup), .waves, .nimg (images per tile), .grid; tail forward also .spl (lanes per (row,
    head) pair of the cross-attention); tail backward .mf (MFMA key-gradient form) and .tpi."""

    def __init__(self, **kw):
        knobs = [k for k in KNOBS if k in os.environ]
        assert not knobs, (f"{knobs} set in the environment: StPlan copies the dispatch at its default knobs, so the "
                           "path a case asserts would not be the path the library takes")
        self.__dict__.update(kw)

    def key(self):
        return tuple(self.__dict__.get(k) for k in ("entry", "c", "tile", "waves", "mf")) if self.rc == OK else None

    @staticmethod
    def stats_add(c, rows, r32_c64=False, stats_add=True):
        """ops.st_tail_fwd's choice of the add form (two 32-row tiles per statistics slot)"""
        return bool(((c == 128 and rows // 64 < 256) or (c == 64 and r32_c64)) and stats_add)

    @staticmethod
    def _tile_ok(R, rows, tokens):
        return rows % R == 0 and (R % tokens == 0 or tokens % R == 0)

    @classmethod
    def tail_fwd(cls, c, rows, tokens, nctx, gn_stats=False, add=False, head=False, heads=8):
        e = "tail_fwd"
        if heads != 8 or c not in (64, 128, 256):
            return cls(entry=e, rc=ERR_UNSUPPORTED)
        if nctx < 1 or nctx > 64 or tokens < 1 or rows < 1 or rows % tokens:
            return cls(entry=e, rc=ERR_SHAPE)
        if gn_stats and (c == 256 or rows % 64):
            return cls(entry=e, rc=ERR_SHAPE)

        def launch(R):
            waves = 4
            if c == 128 and rows // R < 256:
                waves = 8
            if c == 256 and R == 16 and head and rows // R < 256:
                waves = 8
            if not cls._tile_ok(R, rows, tokens):
                return cls(entry=e, rc=ERR_SHAPE)
            nimg = R // tokens if R > tokens else 1
            if tail_fwd_lds(c, R, nimg, nctx) > LDS_MAX:
                return cls(entry=e, rc=ERR_SHAPE)
            nth, npr = 64 * waves, R * 8
            spl = 4 if nth // npr >= 4 else (2 if nth // npr >= 2 else 1)
            return cls(entry=e, rc=OK, c=c, tile=R, waves=waves, nimg=nimg, grid=rows // R, spl=spl, mf=None)
        if gn_stats and add and c == 128 and rows // 64 < 256:
            return launch(32)
        if gn_stats and add and c == 64:
            return launch(32)
        rdef = 32 if c == 256 else 64
        if gn_stats or rows // rdef >= 256:
            p = launch(rdef)
            if p.rc != ERR_SHAPE or gn_stats:
                return p
        return launch(16)

    @classmethod
    def head_fwd(cls, c, rows, tokens, in_stats=False, n1=False, self_stats=False):
        e = "head_fwd"
        if c not in (64, 128, 256):
            return cls(entry=e, rc=ERR_UNSUPPORTED)
        if tokens < 1 or rows < 1 or rows % tokens:
            return cls(entry=e, rc=ERR_SHAPE)
        if c == 256 and (rows // 16 >= 256 or n1):
            return cls(entry=e, rc=ERR_SHAPE)
        if in_stats and tokens % 64:
            return cls(entry=e, rc=ERR_SHAPE)

        def launch(R, waves):
            if not cls._tile_ok(R, rows, tokens):
                return cls(entry=e, rc=ERR_SHAPE)
            nimg = R // tokens if R > tokens else 1
            if head_fwd_lds(c, R, nimg, waves, self_stats) > LDS_MAX:
                return cls(entry=e, rc=ERR_SHAPE)
            return cls(entry=e, rc=OK, c=c, tile=R, waves=waves, nimg=nimg, grid=rows // R, mf=None)
        if rows // 64 >= 256:
            p = launch(64, 4)
            if p.rc != ERR_SHAPE:
                return p
        if c == 128 and rows // 32 >= 256:
            p = launch(32, 4)
            if p.rc != ERR_SHAPE:
                return p
        return launch(16, 8 if c == 256 else 4)

    @staticmethod
    def tail_bwd_tile(c, rows, tokens):
        """encdiff_st_tail_bwd_tile"""
        if c == 64:
            return 64
        return 64 if rows // 64 >= 256 and tokens % 64 == 0 else 32

    @classmethod
    def tail_bwd(cls, c, rows, tokens, nctx, part_rows=None, heads=8):
        e = "tail_bwd"
        if heads != 8 or c not in (64, 128):
            return cls(entry=e, rc=ERR_UNSUPPORTED)
        part_rows = rows if part_rows is None else part_rows
        if nctx < 1 or nctx > 64 or tokens < 1 or rows < 1 or rows % tokens or part_rows < 1:
            return cls(entry=e, rc=ERR_SHAPE)
        R = cls.tail_bwd_tile(c, rows, tokens)
        if tokens % R or rows % R or rows // R > part_rows:
            return cls(entry=e, rc=ERR_SHAPE)
        if (rows // R) * nctx * 2 * c * 4 >= 0x7FFFFFF0:
            return cls(entry=e, rc=ERR_SHAPE)
        mf = tail_bwd_mf(c, R, nctx)
        if tail_bwd_lds(c, R, nctx, mf) > LDS_MAX:
            return cls(entry=e, rc=ERR_SHAPE)
        return cls(entry=e, rc=OK, c=c, tile=R, waves=4, nimg=1, grid=rows // R, mf=mf, tpi=tokens // R)

    @classmethod
    def head_bwd(cls, c, rows, part_rows=None):
        e = "head_bwd"
        if c not in (64, 128):
            return cls(entry=e, rc=ERR_UNSUPPORTED)
        part_rows = rows if part_rows is None else part_rows
        if rows < 1 or part_rows < 1:
            return cls(entry=e, rc=ERR_SHAPE)
        R = 64 if (c == 64 and rows % 64 == 0 and rows // 64 >= 256) else 32
        if rows % R or rows // R > part_rows:
            return cls(entry=e, rc=ERR_SHAPE)
        return cls(entry=e, rc=OK, c=c, tile=R, waves=4, nimg=1, grid=rows // R, mf=None)


def reachable():
    """Every (entry, c, tile, waves, mf) the dispatch can produce, over the shapes that matter: tokens a
    power of four up to 1024, batches a power of two up to 8192 (rows <= 65536), n_ctx 1 .. 64, every
    statistics / head form."""
    seen = set()
    for c in (64, 128, 256):
        for tokens in (1, 4, 16, 32, 64, 256, 1024):
            for lb in range(14):
                rows = tokens << lb
                if rows > 65536:
                    break
                for nctx in (1, 20, 40, 64):
                    for gs, add, head in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1)):
                        seen.add(StPlan.tail_fwd(c, rows, tokens, nctx, bool(gs), bool(add), bool(head)).key())
                for ins, n1, ss in ((0, 0, 0), (1, 1, 0), (0, 0, 1), (0, 1, 0)):
                    seen.add(StPlan.head_fwd(c, rows, tokens, bool(ins), bool(n1), bool(ss)).key())
                for nctx in range(1, 65):
                    seen.add(StPlan.tail_bwd(c, rows, tokens, nctx).key())
                seen.add(StPlan.head_bwd(c, rows).key())
    seen.discard(None)
    return seen
