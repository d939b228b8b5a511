"""Pure-torch restatements of softmax attention as csrc/attn_mfma.hip and the two attention kernels
of csrc/fp32.hip define it (include/encdiff_hip.h: EncdiffAttnArgs), and a Python copy of the launch
planner of attn_mfma.hip.  tests/test_gpu_attention.py compares the HIP kernels with them;
tests/test_attn_restate.py checks the restatements on the CPU against torch autograd in fp64 and the
planner copy against shapes worked by hand.

Tensors here are split by head: [B * heads][S][dh] (split_heads / merge_heads convert from and to
the rows [B * S][heads * dh] the kernels see).  Everything takes a `dtype`: evaluated in fp64 it is
the reference, in fp32 the "torch fp32 evaluation" whose distance from fp64 sets the additive floor
of the comparison rules (tests/elementwise_restate.py).

The planner copy assumes the default tuning knobs (ENCDIFF_ATTN_DSL_MAX, ENCDIFF_ATTN_KCHUNK,
ENCDIFF_ATTN_SPLIT unset); the GPU module refuses to run with one of them set.
"""

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E4M3 = torch.float8_e4m3fn

OK, ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -3
LOG2E = 1.4426950408889634
FWD_BOUND_MAX = 40.0
KNOBS = ("ENCDIFF_ATTN_DSL_MAX", "ENCDIFF_ATTN_KCHUNK", "ENCDIFF_ATTN_SPLIT")


def split_heads(t, B, S, H, dh):
    """rows [B * S][H * dh] -> [B * H][S][dh]"""
    return t.reshape(B, S, H, dh).permute(0, 2, 1, 3).reshape(B * H, S, dh)


def merge_heads(t, B, S, H, dh):
    """[B * H][S][dh] -> rows [B * S][H * dh]"""
    return t.reshape(B, H, S, dh).permute(0, 2, 1, 3).reshape(B * S, H * dh)


# ------------------------------------------------------------------ restatements
def _scores(q, k, scale, fp8, dtype):
    if fp8:  # the score operands rounded to OCP e4m3; every other product uses the given q, k
        q, k = q.to(E4M3), k.to(E4M3)
    return q.to(dtype) @ k.to(dtype).transpose(1, 2) * scale


def attn_fwd(q, k, v, scale, fp8=False, dtype=F64):
    """o = softmax(q k^T scale) v and the natural-log LSE of the scaled scores, per head.
    Returns o, lse and abs_o = att |v| (what a relative error of every p moves o by)."""
    s = _scores(q, k, scale, fp8, dtype)
    lse = torch.logsumexp(s, -1)
    att = torch.exp(s - lse[..., None])
    v = v.to(dtype)
    return dict(o=att @ v, lse=lse, abs_o=att @ v.abs())


def attn_bwd(q, k, v, o_in, lse_in, d_o, scale, fp8=False, dtype=F64):
    """The backward from its givens, as the kernels define it: P = exp(s - lse_in), D = rowsum(d_o
    o_in) from the o it is handed, dS = P (d_o v^T - D); dq = dS k scale, dk = dS^T q scale,
    dv = P^T d_o.  Also the absolute-value contractions P^T |d_o|, |dS|^T |q| scale, |dS| |k| scale."""
    s = _scores(q, k, scale, fp8, dtype)
    q, k, v, o_in, lse_in, d_o = (t.to(dtype) for t in (q, k, v, o_in, lse_in, d_o))
    P = torch.exp(s - lse_in[..., None])
    D = (d_o * o_in).sum(-1, keepdim=True)
    dS = P * (d_o @ v.transpose(1, 2) - D)
    Pt, dSt = P.transpose(1, 2), dS.transpose(1, 2)
    return dict(dq=dS @ k * scale, dk=dSt @ q * scale, dv=Pt @ d_o,
                abs_dq=dS.abs() @ k.abs() * scale, abs_dk=dSt.abs() @ q.abs() * scale, abs_dv=Pt @ d_o.abs(),
                round_dv=(Pt.to(BF16).to(dtype) - Pt).abs() @ d_o.abs())


def dv_p_slack(b64):
    """The P term of dv's bound.  The rule allows 2^-9 (P^T |dO|): half of bf16's worst case, which a sum
    over many queries never approaches.  Where one or two queries carry a key's whole column (few
    queries, a peaked softmax) nothing averages: the element's error IS the rounding error of those
    p, up to 2^-8 p each (bf16 keeps 8 significant bits).  round_dv is that error taken exactly,
    |bf16(P) - P|^T |dO| from the fp64 P, so the term is max(2^-9 P^T |dO|, |bf16(P) - P|^T |dO|): no
    constant is widened, and an element whose p round well gains nothing."""
    return torch.maximum(2.0 ** -9 * b64["abs_dv"], b64["round_dv"])


def fp8_lse_slack(q, k, scale):
    """What v_mfma_f32_16x16x32_fp8_fp8 may move the lse by, per query row [BH][sq], in fp64.

    The instruction does not add its 32 products in fp32.  Measured with a stand-alone program on the
    MI355X (operands powers of two, one 16x16x32 MFMA): within each group of 8 consecutive k the
    products are aligned to the group's largest, 2^E <= max |product| < 2^(E+1), and every product is
    truncated to a multiple of 2^(E-13) -- 2^16 + 2^(16-d) is exact for d <= 13 and gives 2^16 for
    d >= 14; 2^16 + 1.875^2 2^3 gives 2^16 + 24, not 28.125; of 31 products of 2^2 next to one of
    2^16 exactly the 7 sharing its group vanish.  The four group sums and C are then added exactly
    as fp32 (a small product in another group, or in C, survives down to 2^-23 of the sum).
    So a score is off by less than 2^(E_g - 13) for every product of group g that is no multiple of
    that (an e4m3 product has 8 significant bits: only products below 2^-6 of the group's largest
    lose anything), D_ij = scale sum_g 2^(E_g - 13) #{such products}, and lse moves by at most
    log sum_j p_j exp(D_ij) = logsumexp(s + D) - logsumexp(s)."""
    q8, k8 = q.to(E4M3).to(F64), k.to(E4M3).to(F64)
    BH, sq, dh = q8.shape
    assert dh % 8 == 0
    prod = (q8[:, :, None, :] * k8[:, None, :, :]).abs().reshape(BH, sq, k8.shape[1], dh // 8, 8)
    mx = prod.amax(-1, keepdim=True)
    gran = torch.where(mx > 0, torch.exp2(torch.floor(torch.log2(mx.clamp_min(1e-300))) - 13), torch.ones_like(mx))
    lossy = (torch.remainder(prod, gran) != 0).sum(-1, keepdim=True)
    D = (gran * lossy).sum((-1, -2)) * scale
    s = q8 @ k8.transpose(1, 2) * scale
    return torch.logsumexp(s + D, -1) - torch.logsumexp(s, -1)


def row_bounds(q, k, scale):
    """The forward's score bound of every query row, computed as the kernel does, in fp32:
    sqrt(|q|^2 max_k |k|^2) scale log2e 1.001 + 1e-6 (log2 domain).  q, k split by head; [BH][sq]."""
    n2 = (q.float() ** 2).sum(-1)
    k2 = (k.float() ** 2).sum(-1).amax(-1, keepdim=True)
    sl2 = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    return torch.sqrt(n2 * k2) * sl2 * 1.001 + 1e-6


def task_on_bound_path(bounds, nt):
    """[BH][tasks] bool: a wave task (nt 16-query tiles of one head) takes the bound path only if
    every row of every tile is within FWD_BOUND_MAX."""
    BH, sq = bounds.shape
    rows = nt * 16
    ntask = (sq + rows - 1) // rows
    b = torch.zeros(BH, ntask * rows, dtype=bounds.dtype, device=bounds.device)
    b[:, :sq] = bounds
    return (b.reshape(BH, ntask, rows) <= FWD_BOUND_MAX).all(-1)


# ------------------------------------------------------------------ launch planner (a copy of attn_mfma.hip's)
LDS_MAX = 160 * 1024
DSL_MAX = 52 * 1024   # ENCDIFF_ATTN_DSL_MAX default
KCHUNK = 64           # ENCDIFF_ATTN_KCHUNK default


def mfma_hpb(sq, heads):
    hpb = 1 if sq >= 64 else 4
    while hpb > 1 and heads % hpb:
        hpb >>= 1
    return hpb


def attn_qsplit(ktiles, hpb):
    t = ktiles * hpb
    return 1 if t >= 4 else (2 if t >= 2 else 4)


def ds_pitch(sqp):
    return sqp + 16


def fwd_tiles_per_task(dh):
    return 4 if dh == 8 else 2


class AttnPlan:
    """What encdiff_attention_fwd / _bwd (bf16) do with a shape.  fwd_rc / bwd_rc: the return code;
    the fwd_* / bwd_* fields exist when the respective code is OK."""

    def __init__(self, batch, heads, sq, sk, dh, fp8=False):
        self.fwd_rc = self.bwd_rc = self._refusal(batch, heads, sq, sk, dh, fp8)
        if self.fwd_rc != OK:
            return
        if dh == 128:
            self.bwd_rc = ERR_UNSUPPORTED
        self._forward(batch, heads, sq, sk, dh, fp8)
        if self.bwd_rc == OK:
            self._backward(batch, heads, sq, sk, dh, fp8)

    @staticmethod
    def _refusal(batch, heads, sq, sk, dh, fp8):
        if batch <= 0 or heads <= 0 or sq <= 0 or sk <= 0 or dh % 8:
            return ERR_SHAPE
        if batch * heads % mfma_hpb(sq, heads):
            return ERR_SHAPE
        if dh == 128:
            return ERR_UNSUPPORTED if fp8 else OK
        return OK if dh in (8, 16, 32, 64) else ERR_UNSUPPORTED

    def _forward(self, batch, heads, sq, sk, dh, fp8):
        DP = 16 if dh < 16 else dh
        hpb = mfma_hpb(sq, heads)
        SKP = (sk + 31) & ~31
        NT = fwd_tiles_per_task(dh)
        npairs = (((sq + 15) >> 4) + NT - 1) // NT
        lds = hpb * 2 * SKP * DP * 2 + 16 * 4
        kch, nqb = SKP, 1
        self.fwd_hpb_fallback = lds > LDS_MAX
        if lds > LDS_MAX:
            hpb = 1
            kch = (64 * 1024 // (2 * DP * 2)) & ~31
            if kch < 32:
                self.fwd_rc = ERR_SHAPE
                return
            nqb = (npairs + 3) // 4
            lds = 2 * kch * DP * 2 + 16 * 4
        if nqb == 1 and dh >= 64 and hpb == 1:
            nx = batch * heads
            while nqb * 2 * nx <= 256 and npairs >= 4 * nqb * 2:
                nqb *= 2
        self.fwd_hpb, self.fwd_kch, self.fwd_nqb, self.fwd_npairs, self.fwd_lds = hpb, kch, nqb, npairs, lds
        self.fwd_grid = (batch * heads // hpb, nqb)
        self.fwd_sc256 = dh == 8 and not fp8 and sq == 256 and sk == 256 and hpb == 1 and nqb == 1
        self.fwd_mask = sk % 32 != 0 and not self.fwd_sc256
        self.fwd_streamed = min(kch, SKP) != SKP
        self.fwd_bound_eligible = not self.fwd_streamed and not fp8 and dh <= 32
        # bytes the kernel itself addresses: K, V of the resident rows, and the key norms behind
        # them on the resident branch
        KR = min(kch, SKP)
        self.fwd_lds_used = hpb * 2 * KR * DP * 2 + (0 if self.fwd_streamed else 4 * hpb)
        # resident: workgroup y's wave w runs tasks y + nqb (w + 4 j); streamed: task 4 y + w.  Waves
        # (of all the head group's workgroups) left without a task in the last round:
        self.fwd_idle_waves = -(npairs if self.fwd_streamed else hpb * npairs) % (4 * nqb)
        self.fwd_last_chunk = SKP - (SKP - 1) // KR * KR

    def _backward(self, batch, heads, sq, sk, dh, fp8):
        DP = 16 if dh < 16 else dh
        RP = 8 if dh < 16 else dh
        hpb = mfma_hpb(sq, heads)
        SQP, SKP = (sq + 15) & ~15, (sk + 15) & ~15
        QS = attn_qsplit(SKP // 16, hpb)
        red = hpb * (SKP // 16) * QS * 2 * 16 * DP * 4 if QS > 1 else 0
        base = hpb * ((2 * SQP + 2 * SKP) * RP * 2 + 2 * SQP * 4) + red
        dsz = hpb * SKP * ds_pitch(SQP) * 2
        dsl = 1 if base + dsz <= DSL_MAX else 0
        lds = base + (dsz if dsl else 0)
        if not dsl and KCHUNK >= 16 and hpb == 1 and QS == 1 and SQP <= 256 and SKP > KCHUNK:
            csz = KCHUNK * ds_pitch(SQP) * 2
            if base + csz <= DSL_MAX + 4096:
                dsl = KCHUNK & ~15
                lds = base + csz
        self.bwd_lds = lds
        if lds > LDS_MAX:
            self.bwd_rc = ERR_SHAPE
            return
        self.bwd_hpb, self.bwd_qs, self.bwd_dsl = hpb, QS, dsl
        self.bwd_sc256 = dh == 8 and not fp8 and sq == 256 and sk == 256 and hpb == 1 and dsl != 1
        self.bwd_mask = (sq % 16 != 0 or sk % 16 != 0) and not self.bwd_sc256
        if dsl == 1:
            self.bwd_mode = "lds"
        elif dsl == 0:
            self.bwd_mode = "recompute"
        else:
            self.bwd_mode = "chunk_swz" if SQP & 255 == 0 else "chunk"
        self.bwd_qtiles, self.bwd_ktiles = SQP // 16, SKP // 16
        # phase A's loop form (not on the chunked path, which pairs consecutive tiles)
        self.bwd_loop_even = (SQP // 16) % (2 * QS) == 0
        self.bwd_last_chunk_tiles = ((SKP - 1) % dsl + 1) // 16 if dsl > 1 else 0

    def bwd_key(self):
        return (self.bwd_mode, self.bwd_qs, self.bwd_mask, self.bwd_hpb)


def reachable_bwd(smax=1024, dhs=(8, 16, 32, 64), heads=(1, 2, 3, 4)):
    """Every (mode, QS, MASK, hpb) the backward planner can produce for sq, sk <= smax (step 1 up to
    80, then the values around every multiple of 16 that matter: s - 1, s, s + 1 for s % 64 == 0)."""
    sizes = sorted(set(range(1, 81)) | {s + d for s in range(64, smax + 1, 64) for d in (-1, 0, 1) if s + d <= smax})
    seen = {}
    for dh in dhs:
        for h in heads:
            for sq in sizes:
                for sk in sizes:
                    p = AttnPlan(1, h, sq, sk, dh)
                    if p.bwd_rc == OK:
                        seen.setdefault(p.bwd_key(), (h, sq, sk, dh))
    return seen
