"""Per-element tests of MFMA attention on the MI355X: csrc/attn_mfma.hip (bf16 and fp8-score forward
and backward, every launch path) and the fp32 attention entries of csrc/fp32.hip.

Reference = tests/attn_restate.py evaluated in fp64 on the case's own (already rounded) inputs;
floor = 4 x the largest |the same restatement in fp32 - fp64| (tests/elementwise_restate.py).
Bounds, derived from where the kernel rounds (p and dS are rounded to bf16 before their MFMAs, every
sum is fp32, the outputs are rounded to bf16 once):
  * o:        |o - ref| <= 2 x 2^-9 (att |v|) + 2^-8 |ref| + floor   (p rounded; at dh 8 the denominator
                                                                    is a sum of the rounded p)
  * lse:      |lse - ref| <= floor + 2^-22 |ref| (+ 2^-9 at dh 8: the denominator's relative error)
  * dv:       2^-9 (P^T |dO|) + 2^-8 |ref| + floor
  * dk, dq:   2 x 2^-9 (|dS|^T |q| scale, |dS| |k| scale) + 2^-8 |ref| + floor
  * fp32 entries: the fp32 rule, floor + 2^-22 |ref|
q, k, v are column views of a fused qkv buffer (sq == sk) or q of its own and a fused kv buffer
(cross), whose rows end in 8 NaN columns; o, dq, dk, dv are views in sentinel-filled buffers, lse in
a NaN-filled one, and everything outside the views must stay unchanged.  Each launch runs twice and
must agree bitwise (the QS partials are summed in slice order; there are no float atomics).  The
backward is fed o (bf16) and lse (fp32) rounded from the fp64 reference; test_chained feeds it the
kernel's own forward outputs.  Every case asserts the launch path it means to reach through
attn_restate.AttnPlan, the copy of the launch planner -- if the planner changes, the case fails
instead of testing nothing.  AttnPlan assumes the default tuning knobs, so the module refuses to run
with ENCDIFF_ATTN_DSL_MAX, ENCDIFF_ATTN_KCHUNK or ENCDIFF_ATTN_SPLIT set.  The ENCDIFF_ATTN_SPLIT
branch (phase A and B in workgroups of their own) is off by default and read once per process; it is
not covered here.

Two derived additions, no constant widened (both in attn_restate.py, with their derivations):
  * dv: the P term is max(2^-9 P^T |dO|, |bf16(P) - P|^T |dO|) (dv_p_slack).  With 16 queries and a
    peaked column one p carries an element of dv, and its bf16 rounding (up to 2^-8, the format's
    worst case; the rule's 2^-9 is half of it) does not average out: [rc-qs1-mask-hpb2] (sq 16, sk 90,
    dh 64) exceeded the plain rule by 2.5e-5 at |error| 1.9e-3 in one of 11520 elements.
  * fp8 lse: v_mfma_f32_16x16x32_fp8_fp8 truncates every product to 2^-13 of the largest of its group
    of 8 (measured with a stand-alone program, see fp8_lse_slack), so the scores themselves are off
    by up to ~1e-4 and the lse by up to 2.3e-5 where the fp32 floor is 2e-6.  fp8_lse_slack bounds that
    per row from the e4m3 operands (up to 1.3e-4 here); the bf16 paths keep the plain rule.
Largest floors measured on the MI355X (the whole file, 103 cases, takes about 5 s):
  bf16: o 2.4e-5 and lse 3.1e-5 (both at q x 12; 2.7e-6 at q x 1), dq 3.3e-6, dk 6.0e-6, dv 1.3e-5
  fp8 scores: o 1.8e-6, lse 2.7e-6, dq 1.7e-6, dk 1.6e-6, dv 1.9e-6
  fp32 entries: lse 2.8e-6, dq 2.9e-6, dk 2.2e-6, dv 1.9e-6
  (largest errors: o 9.8e-3, lse 1.7e-3 at dh 8 -- the denominator from rounded p -- and 3.3e-6 elsewhere,
  dq 1.1e-2, dk 1.8e-2, dv 2.0e-2; the closest any lse comes to its bound is 4.6e-7, under the loose bound)

Kernel branch -> test
  forward, hpb 4 (one key step; three query tiles: a half-empty pair) ........ test_fwd[hpb4-*]
  forward, hpb 2 / hpb 1 below 64 queries (heads % 4 != 0) .................... test_fwd[hpb2-*], [hpb1-h3-*]
  dh 8 four-tile task with 3 / 2 invalid tiles, sk 31 / 32 / 33 ............... test_fwd[dh8-72x*], [dh8-80x*]
  SC256, grid 1 (identity) and 8 (XCD remap) .................................. test_fwd[sc256-h1], [sc256-h8]
  dh 16 / 32 / 64, unmasked and masked with sq % 16 != 0 ...................... test_fwd[dh16-*], [dh32-*], [dh64-*]
  resident forward over blockIdx.y (nqb 2), dh 128 / 64, idle waves at 272 .... test_fwd[nqb2-*]
  streamed K / V: sk % 32 != 0, last chunk of 32 rows with masked keys, dh 64
    with a 160-row last chunk, dh 8 through the hpb fallback (ONES, r0 != 0) .. test_fwd[streamed-*]
  fp8 scores: dh 16 (KC8 1, zero fragment half), 32, 64 (KC8 2), masked ....... test_fwd[fp8-*]
  bound path (diffuse), running max, a task whose tiles disagree, a bound
    loose by ~35 in the log2 domain .......................................... test_fwd_bound
  hpb fallback that stays resident (SKP == kch: kn behind 64 KB of K / V) ..... test_fwd_fallback_resident
  refusals (dh 12 / 24, dh 128 backward / fp8, backward LDS > 160 KB) ......... test_refusals
  fp32 entries, masked tails ................................................. test_f32
  forward -> backward on the kernel's own o / lse ............................ test_chained
  backward (mode, QS, MASK, hpb) -- every combination reachable for sq, sk <= 1024
  (attn_restate.reachable_bwd; test_attn_restate.py pins the list):
    lds       1 - 1 / 2 / 4   test_bwd[lds-qs1-hpb1-dh64], [lds-qs1-hpb2], [lds-qs1-hpb4]
    lds       1 M 1 / 2 / 4   test_bwd[lds-qs1-mask-hpb1], [lds-qs1-mask-hpb2], [lds-qs1-mask-hpb4-4x4], [lds-qs1-mask-hpb4-48x40]
    lds       2 - 1 / 2       test_bwd[lds-qs2-hpb1], [lds-qs2-hpb1-even], [lds-qs2-hpb2]
    lds       2 M 1 / 2       test_bwd[lds-qs2-mask-hpb1-h3], [lds-qs2-mask-hpb1-sk20], [lds-qs2-mask-hpb1-72x31],
                              [lds-qs2-mask-hpb2]
    lds       4 - / M  1      test_bwd[lds-qs4-dh8], [lds-qs4-dh32], [lds-qs4-even], [lds-qs4-mask-dh8],
                              [lds-qs4-mask-dh32]
    recompute 1 - 1 / 2 / 4   test_bwd[rc-qs1-hpb1-1024-dh16], [rc-qs1-hpb1-1024-dh16-fp8], [rc-qs1-hpb1-256-dh16],
                              [rc-qs1-hpb2], [rc-qs1-hpb4]
    recompute 1 M 1 / 2 / 4   test_bwd[rc-qs1-mask-hpb1], [rc-qs1-mask-hpb2], [rc-qs1-mask-hpb4]
    recompute 2 - 1 / 2       test_bwd[rc-qs2-hpb1], [rc-qs2-hpb2]
    recompute 2 M 1 / 2       test_bwd[rc-qs2-mask-hpb1-512x20], [rc-qs2-mask-hpb1-dh64-16x40], [rc-qs2-mask-hpb2]
    recompute 4 - / M  1      test_bwd[rc-qs4], [rc-qs4-mask]
    chunk     1 - / M  1      test_bwd[chunk-128x256], [chunk-dh16], [chunk-mask-120x200] (last chunk one tile)
    chunk_swz 1 - / M  1      test_bwd[swz-256x80], [swz-sc256-h1], [swz-sc256-h8], [swz-mask-256x77] (last chunk
                              one tile), [swz-mask-250x256]
    unreachable: lds / recompute with QS 4 and hpb > 1, QS 2 and hpb 4 (QS > 1 needs ktiles x hpb < 4);
      chunk / chunk_swz with QS > 1 or hpb > 1 (the planner's own condition).  256 x 256 at dh 16
      recomputes (its staging alone leaves no room for a chunk): chunk_swz exists at dh 8 only.
    phase A loop forms: qtiles % (2 QS) == 0 in [lds-qs2-hpb1-even], [lds-qs4-even], [rc-qs2-*]; != 0 in
      [lds-qs4-dh8], [lds-qs2-mask-hpb1-72x31], [rc-qs1-hpb4] (asserted as bwd_loop_even)
    fp8 backward: test_bwd[fp8-*], [rc-qs1-hpb1-1024-dh16-fp8]
"""
import os

import pytest
import torch

import attn_restate as A
import elementwise_restate as R
from test_gpu_elementwise import Guard, place, rnd, _gen, assert_f32_rule

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    knobs = [k for k in A.KNOBS if k in os.environ]
    assert not knobs, (f"{knobs} set in the environment: attn_restate.AttnPlan copies the planner at its default "
                       "knobs, so the path every case asserts would not be the path the library takes")
    from encdiff_amd import ops
    return ops


def nan_guard(rows, cols):
    return Guard(rows, cols, F32, init=torch.full((rows, cols), NAN, device=dev))


def expect_plan(p, **want):
    for k, v in want.items():
        assert getattr(p, k) == v, f"launch plan changed: {k} = {getattr(p, k)}, this case needs {v}"


class Inputs:
    """q, k, v rows as the kernels get them: views of fused buffers whose rows end in 8 NaN columns."""

    def __init__(self, B, H, sq, sk, dh, q, k, v, fp8=False):
        self.shape = (B, H, sq, sk, dh)
        self.fp8 = fp8
        self.scale = dh ** -0.5
        C = H * dh
        dt = q.dtype
        if sq == sk:  # self-attention: one fused qkv projection
            buf = torch.full((B * sq, 3 * C + 8), NAN, dtype=dt, device=dev)
            buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:3 * C] = q, k, v
            self.q, self.k, self.v = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:3 * C]
            self.bufs = [buf]
        else:         # cross-attention: q of its own, fused kv
            buf = torch.full((B * sk, 2 * C + 8), NAN, dtype=dt, device=dev)
            buf[:, :C], buf[:, C:2 * C] = k, v
            qg = Guard(B * sq, C, dt, strided=True, init=q)
            self.q, self.k, self.v = qg.view, buf[:, :C], buf[:, C:2 * C]
            self.bufs = [buf, qg.buf]
        self.before = [b.clone() for b in self.bufs]

    def unchanged(self):
        assert all(R.same_bits(a, b) for a, b in zip(self.bufs, self.before)), "an input buffer was written"

    def split(self, t, s):
        B, H, _, _, dh = self.shape
        return A.split_heads(t, B, s, H, dh)

    def heads(self):
        _, _, sq, sk, _ = self.shape
        return self.split(self.q, sq), self.split(self.k, sk), self.split(self.v, sk)


def randn_inputs(seed, B, H, sq, sk, dh, fp8=False, qscale=1.0, dtype=BF16):
    g = _gen(seed)
    C = H * dh
    return Inputs(B, H, sq, sk, dh, rnd(g, B * sq, C, scale=qscale, dtype=dtype), rnd(g, B * sk, C, dtype=dtype),
                  rnd(g, B * sk, C, dtype=dtype), fp8)


def assert_bound(out, ref64, t32, slack, rel, what):
    """|out - ref64| <= slack + rel |ref64| + floor per element; floor from the fp32 evaluation."""
    floor = R.floor_of(t32, ref64)
    err = (out.double() - ref64).abs()
    ex = err - (slack + rel * ref64.abs() + floor)
    worst = ex.max().item()
    print(f"{what}: floor {floor:.3e} max|out-ref| {err.max().item():.3e} excess {worst:.3e}")
    assert not torch.isnan(out).any(), f"{what}: NaN (unwritten or poisoned) in the output"
    assert worst <= 0, f"{what}: element {int(ex.argmax())} exceeds the bound by {worst:.3e}"


def same_twice(a, b, what):
    for x, y, n in zip(a, b, what):
        assert R.same_bits(x.buf, y.buf), f"{n}: two launches on the same inputs differ bitwise"


# ====================================================================== forward
def fwd_refs(c):
    qs, ks, vs = c.heads()
    return A.attn_fwd(qs, ks, vs, c.scale, c.fp8, F64), A.attn_fwd(qs, ks, vs, c.scale, c.fp8, F32)


def run_fwd(O, c):
    B, H, sq, sk, dh = c.shape
    outs = []
    for _ in range(2):
        o = Guard(B * sq, H * dh, BF16, strided=True)
        lse = nan_guard(B * H, sq)
        O.attention_fwd(c.q, c.k, c.v, o.view, lse.view, B, H, sq, sk, dh, fp8=c.fp8)
        torch.cuda.synchronize()
        o.check()
        lse.check()
        outs.append((o, lse))
    same_twice(outs[0], outs[1], ("o", "lse"))
    c.unchanged()
    return outs[0]


def check_fwd(c, o, lse, refs, what):
    B, H, sq, sk, dh = c.shape
    r64, r32 = refs
    assert_bound(c.split(o.view, sq), r64["o"], r32["o"], 2 * 2.0 ** -9 * r64["abs_o"], 2.0 ** -8, what + " o")
    slack = 2.0 ** -9 if dh == 8 else 0.0
    if c.fp8:  # the fp8 MFMA truncates small products inside a group of 8: derived in fp8_lse_slack
        slack = A.fp8_lse_slack(*c.heads()[:2], c.scale)
        print(f"{what}: fp8 MFMA truncation may move lse by up to {slack.max().item():.3e}")
    assert_bound(lse.view.reshape(B * H, sq), r64["lse"], r32["lse"], slack, 2.0 ** -22, what + " lse")


def fwd_case(O, c, what, refs=None):
    refs = refs or fwd_refs(c)
    o, lse = run_fwd(O, c)
    check_fwd(c, o, lse, refs, what)
    return o, lse, refs


FWD = {  # name: (B, heads, sq, sk, dh, fp8, expected plan fields)
    "hpb4-4x4-dh32": (2, 4, 4, 4, 32, False, dict(fwd_hpb=4, fwd_mask=True, fwd_npairs=1)),
    "hpb4-48x40-dh16": (2, 4, 48, 40, 16, False, dict(fwd_hpb=4, fwd_mask=True, fwd_npairs=2)),
    "hpb2-16x20-dh8": (2, 2, 16, 20, 8, False, dict(fwd_hpb=2, fwd_mask=True)),
    "hpb1-h3-16x33-dh16": (2, 3, 16, 33, 16, False, dict(fwd_hpb=1, fwd_mask=True, fwd_kch=64)),
    "dh8-72x31": (1, 2, 72, 31, 8, False, dict(fwd_hpb=1, fwd_npairs=2, fwd_mask=True)),
    "dh8-72x32": (1, 2, 72, 32, 8, False, dict(fwd_hpb=1, fwd_npairs=2, fwd_mask=False)),
    "dh8-72x33": (1, 2, 72, 33, 8, False, dict(fwd_hpb=1, fwd_npairs=2, fwd_mask=True, fwd_kch=64)),
    "dh8-80x31": (1, 2, 80, 31, 8, False, dict(fwd_hpb=1, fwd_npairs=2, fwd_mask=True)),
    "dh8-80x32": (1, 2, 80, 32, 8, False, dict(fwd_hpb=1, fwd_npairs=2, fwd_mask=False)),
    "dh8-80x33": (1, 2, 80, 33, 8, False, dict(fwd_hpb=1, fwd_npairs=2, fwd_mask=True, fwd_kch=64)),
    "sc256-h1": (1, 1, 256, 256, 8, False, dict(fwd_sc256=True, fwd_grid=(1, 1))),
    "sc256-h8": (1, 8, 256, 256, 8, False, dict(fwd_sc256=True, fwd_grid=(8, 1))),
    "dh16-64x64": (2, 2, 64, 64, 16, False, dict(fwd_hpb=1, fwd_mask=False, fwd_sc256=False)),
    "dh16-70x45": (2, 2, 70, 45, 16, False, dict(fwd_hpb=1, fwd_mask=True)),
    "dh32-32x32": (1, 2, 32, 32, 32, False, dict(fwd_hpb=2, fwd_mask=False)),
    "dh32-37x50": (1, 2, 37, 50, 32, False, dict(fwd_hpb=2, fwd_mask=True)),
    "dh64-64x64": (1, 2, 64, 64, 64, False, dict(fwd_hpb=1, fwd_mask=False, fwd_nqb=1, fwd_bound_eligible=False)),
    "dh64-40x50": (1, 2, 40, 50, 64, False, dict(fwd_hpb=2, fwd_mask=True)),
    "nqb2-256-dh128": (2, 1, 256, 256, 128, False, dict(fwd_nqb=2, fwd_streamed=False, fwd_idle_waves=0)),
    "nqb2-256-dh64": (2, 1, 256, 256, 64, False, dict(fwd_nqb=2, fwd_streamed=False)),
    "nqb2-272-dh128": (2, 1, 272, 272, 128, False, dict(fwd_nqb=2, fwd_streamed=False, fwd_mask=True, fwd_idle_waves=7)),
    "streamed-1000-dh128": (1, 1, 1000, 1000, 128, False, dict(fwd_streamed=True, fwd_kch=128, fwd_mask=True, fwd_nqb=8)),
    "streamed-1048-dh128": (1, 1, 1048, 1048, 128, False, dict(fwd_streamed=True, fwd_last_chunk=32, fwd_mask=True)),
    "streamed-40x650-dh64": (1, 1, 40, 650, 64, False, dict(fwd_streamed=True, fwd_kch=256, fwd_last_chunk=160)),
    "streamed-h4-16x1100-dh8": (1, 4, 16, 1100, 8, False, dict(fwd_streamed=True, fwd_hpb_fallback=True, fwd_hpb=1,
                                                              fwd_last_chunk=96, fwd_grid=(4, 1))),
    "fp8-dh16": (1, 2, 64, 64, 16, True, dict(fwd_mask=False, fwd_bound_eligible=False)),
    "fp8-dh32": (1, 2, 64, 64, 32, True, dict(fwd_mask=False)),
    "fp8-dh64": (1, 2, 64, 64, 64, True, dict(fwd_mask=False)),
    "fp8-mask-72x20-dh16": (1, 2, 72, 20, 16, True, dict(fwd_mask=True, fwd_hpb=1)),
}


@pytest.mark.parametrize("name", list(FWD))
def test_fwd(O, name):
    """One forward launch per path, o and lse per element.  Catches: a masked key leaking into one
    row's denominator (the bound on lse is ~1e-6, a leaked key moves it by 1 / sk or more), invalid
    tiles of a four-tile task stored or their rows' lse written, a head group's second head read
    from the first head's K / V, the key offset of a streamed chunk (r0) dropped from the mask or the
    ONES column, tasks of a blockIdx.y-spread head run twice or not at all, the zero half of an fp8
    fragment filled from the next row."""
    B, H, sq, sk, dh, fp8, want = FWD[name]
    expect_plan(A.AttnPlan(B, H, sq, sk, dh, fp8), fwd_rc=A.OK, **want)
    fwd_case(O, randn_inputs(1000 + sq + sk + dh, B, H, sq, sk, dh, fp8), name)


BOUND_SHAPES = [(2, 4, 48, 40, 16), (1, 2, 80, 33, 8), (2, 4, 16, 20, 32), (1, 1, 256, 256, 8)]


def _bound_inputs(kind, B, H, sq, sk, dh, seed):
    """Inputs whose rows' score bounds (attn_restate.row_bounds: the kernel's own fp32 formula) lie
    where the case wants them; returns (inputs, check of the bounds)."""
    g = _gen(seed)
    C = H * dh
    nt = A.fwd_tiles_per_task(dh)
    q = rnd(g, B * sq, C, dtype=BF16)
    k = rnd(g, B * sk, C, dtype=BF16)
    v = rnd(g, B * sk, C, dtype=BF16)
    if kind == "running_max":
        q = (q.float() * 12).to(BF16)
    elif kind == "mixed":
        # rows 16 .. 31 of every head (the second tile of the first task) x 12; one more single row
        qh = A.split_heads(q.float(), B, sq, H, dh)
        if sq > 16:
            qh[:, 16:32] *= 12
        qh[:, sq - 3 if sq > 32 else 5] *= 16
        q = A.merge_heads(qh, B, sq, H, dh).to(BF16)
    elif kind == "loose":
        # key 1 of every head is c e_0 and every q has q[0] = 0: that key's scores are 0 like many
        # others, but max |k|^2 = c^2, so the bound is |q| c scale log2e ~ 35 while the true scores
        # stay within a few units: every p is ~2^-35, tiny but normal
        qh = A.split_heads(q.float(), B, sq, H, dh)
        qh[..., 0] = 0
        qh = qh / qh.norm(dim=-1, keepdim=True) * 2.0
        q = A.merge_heads(qh, B, sq, H, dh).to(BF16)
        c = float(torch.tensor(35.0 / (2.0 * dh ** -0.5 * A.LOG2E)).to(BF16))
        kh = A.split_heads(k.float(), B, sk, H, dh)
        kh[:, 1] = 0
        kh[:, 1, 0] = c
        k = A.merge_heads(kh, B, sk, H, dh).to(BF16)
    inp = Inputs(B, H, sq, sk, dh, q, k, v)
    qs, ks, _ = inp.heads()
    bounds = A.row_bounds(qs, ks, inp.scale)
    on = A.task_on_bound_path(bounds, nt)
    if kind == "diffuse":
        assert on.all() and bounds.max().item() < A.FWD_BOUND_MAX
    elif kind == "running_max":
        assert not on.any()
    elif kind == "mixed":
        t0 = bounds[:, :16 * nt]
        if sq > 16:
            assert (t0[:, :16] <= A.FWD_BOUND_MAX).all(), "the first tile is to stay below the bound"
            assert (t0[:, 16:32].amax(-1) > A.FWD_BOUND_MAX).all(), "the second tile is to exceed the bound"
        assert not on[:, 0].any()
        assert ((bounds > A.FWD_BOUND_MAX).sum(-1) >= 1).all()
    else:
        assert (bounds > 30).all() and (bounds < A.FWD_BOUND_MAX).all(), (bounds.min().item(), bounds.max().item())
        assert on.all()
        true_max = (qs.double() @ ks.double().transpose(1, 2)).amax(-1) * inp.scale * A.LOG2E
        assert (bounds.double() - true_max).min().item() > 25, "the bound is to be loose by > 25 in the log2 domain"
    print(f"{kind}: row bounds {bounds.min().item():.2f} .. {bounds.max().item():.2f}, "
          f"tasks on the bound path {int(on.sum())} of {on.numel()}")
    return inp


@pytest.mark.parametrize("kind", ["diffuse", "running_max", "mixed", "loose"])
@pytest.mark.parametrize("B,H,sq,sk,dh", BOUND_SHAPES, ids=[f"h{s[1]}-{s[2]}x{s[3]}-dh{s[4]}" for s in BOUND_SHAPES])
def test_fwd_bound(O, B, H, sq, sk, dh, kind):
    """The forward's two softmax offsets.  diffuse: every task's rows have a Cauchy-Schwarz bound
    <= 40 and use it as a fixed offset; running_max: q x 12, every task over it; mixed: one tile of a
    task (and a single row elsewhere) over the bound while its partner is under (the task must take
    the running max as a whole: a per-lane choice would mix offsets inside one MFMA column);
    loose: the bound exceeds the true row maximum by > 25 in the log2 domain (every p ~2^-35 -- still
    normal, which is what the bound path's comment promises to handle).  The bounds are computed on
    the host with the kernel's fp32 formula and asserted to lie where the case needs them.
    Catches: denominators flushed or rounded away under a loose bound, an lse that forgets the
    offset, a bound taken from another head's key norms (hpb 4), the max of |k|^2 including or
    missing rows."""
    p = A.AttnPlan(B, H, sq, sk, dh)
    expect_plan(p, fwd_rc=A.OK, fwd_bound_eligible=True)
    fwd_case(O, _bound_inputs(kind, B, H, sq, sk, dh, 2000 + sq + dh), f"{kind} h{H} {sq}x{sk} dh{dh}")


FALLBACK = [(1, 4, 16, 1024, 8), (1, 4, 16, 1000, 16), (1, 4, 16, 512, 32)]


@pytest.mark.parametrize("qscale", [1, 12], ids=["bound", "running_max"])
@pytest.mark.parametrize("B,H,sq,sk,dh", FALLBACK, ids=[f"{s[3]}-dh{s[4]}" for s in FALLBACK])
def test_fwd_fallback_resident(O, B, H, sq, sk, dh, qscale):
    """Four heads whose K / V exceed 160 KB fall back to one head per workgroup and 64 KB chunks; a
    head of exactly one chunk of padded keys still runs the resident branch, whose key norms live
    behind those 64 KB -- the launch has to allocate them.  With q x 1 the bound path needs the
    norm (a zero there gives an offset of 1e-6 and p up to 2^15: an lse off by the offset, or an
    overflow); with q x 12 the running max must be chosen."""
    p = A.AttnPlan(B, H, sq, sk, dh)
    expect_plan(p, fwd_rc=A.OK, fwd_hpb_fallback=True, fwd_hpb=1, fwd_streamed=False, fwd_bound_eligible=True,
                fwd_lds_used=64 * 1024 + 4)
    assert p.fwd_lds >= p.fwd_lds_used
    c = randn_inputs(3000 + sk, B, H, sq, sk, dh, qscale=qscale)
    qs, ks, _ = c.heads()
    on = A.task_on_bound_path(A.row_bounds(qs, ks, c.scale), A.fwd_tiles_per_task(dh))
    assert on.all() if qscale == 1 else not on.any()
    fwd_case(O, c, f"fallback-resident {sq}x{sk} dh{dh} q x {qscale}")


# ====================================================================== backward
def run_bwd(O, c, o_in, lse_in, d_o):
    B, H, sq, sk, dh = c.shape
    outs = []
    for _ in range(2):
        dq = Guard(B * sq, H * dh, BF16, strided=True)
        dk = Guard(B * sk, H * dh, BF16, strided=True)
        dv = Guard(B * sk, H * dh, BF16, strided=True)
        O.attention_bwd(c.q, c.k, c.v, o_in, lse_in, d_o, dq.view, dk.view, dv.view, B, H, sq, sk, dh, fp8=c.fp8)
        torch.cuda.synchronize()
        for t in (dq, dk, dv):
            t.check()
        outs.append((dq, dk, dv))
    same_twice(outs[0], outs[1], ("dq", "dk", "dv"))
    c.unchanged()
    return outs[0]


def bwd_case(O, c, what, seed, own=None):
    """own: (o, lse) views of the kernel's forward; default: both rounded from the fp64 reference."""
    B, H, sq, sk, dh = c.shape
    qs, ks, vs = c.heads()
    if own is None:
        f64 = A.attn_fwd(qs, ks, vs, c.scale, c.fp8, F64)
        o_in = place(A.merge_heads(f64["o"], B, sq, H, dh).to(BF16), True)
        lse_in = f64["lse"].float().contiguous()
    else:
        o_in, lse_in = own
    d_o = place(rnd(_gen(seed), B * sq, H * dh, dtype=BF16), True)
    before = [t.clone() for t in (o_in, lse_in, d_o)]
    dq, dk, dv = run_bwd(O, c, o_in, lse_in, d_o)
    assert all(R.same_bits(a, b) for a, b in zip((o_in, lse_in, d_o), before)), "o, lse or d_o was written"
    args = (qs, ks, vs, c.split(o_in, sq), lse_in.reshape(B * H, sq), c.split(d_o, sq), c.scale, c.fp8)
    b64, b32 = A.attn_bwd(*args, F64), A.attn_bwd(*args, F32)
    assert_bound(c.split(dv.view, sk), b64["dv"], b32["dv"], A.dv_p_slack(b64), 2.0 ** -8, what + " dv")
    assert_bound(c.split(dk.view, sk), b64["dk"], b32["dk"], 2 * 2.0 ** -9 * b64["abs_dk"], 2.0 ** -8, what + " dk")
    assert_bound(c.split(dq.view, sq), b64["dq"], b32["dq"], 2 * 2.0 ** -9 * b64["abs_dq"], 2.0 ** -8, what + " dq")


def _bw(mode, qs, mask, hpb, **more):
    return dict(bwd_mode=mode, bwd_qs=qs, bwd_mask=mask, bwd_hpb=hpb, **more)


BWD = {  # name: (B, heads, sq, sk, dh, fp8, expected plan fields)
    "lds-qs1-hpb1-dh64": (2, 1, 64, 64, 64, False, _bw("lds", 1, False, 1)),
    "lds-qs1-hpb2": (1, 2, 16, 32, 8, False, _bw("lds", 1, False, 2)),
    "lds-qs1-hpb4": (1, 4, 48, 48, 16, False, _bw("lds", 1, False, 4)),
    "lds-qs1-mask-hpb1": (1, 3, 20, 50, 16, False, _bw("lds", 1, True, 1)),
    "lds-qs1-mask-hpb2": (2, 2, 16, 20, 8, False, _bw("lds", 1, True, 2)),
    "lds-qs1-mask-hpb4-4x4": (2, 4, 4, 4, 32, False, _bw("lds", 1, True, 4)),
    "lds-qs1-mask-hpb4-48x40": (2, 4, 48, 40, 16, False, _bw("lds", 1, True, 4)),
    "lds-qs2-hpb1": (1, 1, 16, 32, 8, False, _bw("lds", 2, False, 1, bwd_loop_even=False)),
    "lds-qs2-hpb1-even": (1, 2, 64, 32, 16, False, _bw("lds", 2, False, 1, bwd_loop_even=True)),
    "lds-qs2-hpb2": (1, 2, 16, 16, 8, False, _bw("lds", 2, False, 2)),
    "lds-qs2-mask-hpb1-h3": (2, 3, 16, 33, 16, False, _bw("lds", 2, True, 1, bwd_loop_even=False)),
    "lds-qs2-mask-hpb1-sk20": (1, 2, 64, 20, 8, False, _bw("lds", 2, True, 1, bwd_loop_even=True)),
    "lds-qs2-mask-hpb1-72x31": (1, 2, 72, 31, 8, False, _bw("lds", 2, True, 1, bwd_loop_even=False, bwd_qtiles=5)),
    "lds-qs2-mask-hpb2": (1, 2, 10, 9, 8, False, _bw("lds", 2, True, 2)),
    "lds-qs4-dh8": (1, 2, 64, 16, 8, False, _bw("lds", 4, False, 1, bwd_loop_even=False)),
    "lds-qs4-dh32": (1, 2, 64, 16, 32, False, _bw("lds", 4, False, 1)),
    "lds-qs4-even": (1, 1, 128, 16, 8, False, _bw("lds", 4, False, 1, bwd_loop_even=True)),
    "lds-qs4-mask-dh8": (1, 2, 64, 9, 8, False, _bw("lds", 4, True, 1)),
    "lds-qs4-mask-dh32": (1, 2, 64, 9, 32, False, _bw("lds", 4, True, 1)),
    "rc-qs1-hpb1-1024-dh16": (1, 1, 1024, 1024, 16, False, _bw("recompute", 1, False, 1)),
    "rc-qs1-hpb1-1024-dh16-fp8": (1, 1, 1024, 1024, 16, True, _bw("recompute", 1, False, 1)),
    "rc-qs1-hpb1-256-dh16": (1, 2, 256, 256, 16, False, _bw("recompute", 1, False, 1)),
    "rc-qs1-hpb2": (1, 2, 16, 96, 64, False, _bw("recompute", 1, False, 2)),
    "rc-qs1-hpb4": (1, 4, 48, 256, 16, False, _bw("recompute", 1, False, 4, bwd_loop_even=False)),
    "rc-qs1-mask-hpb1": (1, 1, 250, 256, 16, False, _bw("recompute", 1, True, 1)),
    "rc-qs1-mask-hpb2": (1, 2, 16, 90, 64, False, _bw("recompute", 1, True, 2)),
    "rc-qs1-mask-hpb4": (1, 4, 40, 250, 16, False, _bw("recompute", 1, True, 4)),
    "rc-qs2-hpb1": (1, 1, 512, 32, 8, False, _bw("recompute", 2, False, 1, bwd_loop_even=True)),
    "rc-qs2-hpb2": (1, 2, 32, 16, 64, False, _bw("recompute", 2, False, 2)),
    "rc-qs2-mask-hpb1-512x20": (1, 1, 512, 20, 8, False, _bw("recompute", 2, True, 1, bwd_loop_even=True)),
    "rc-qs2-mask-hpb1-dh64-16x40": (2, 1, 16, 40, 64, False, _bw("recompute", 2, True, 1, bwd_loop_even=False)),
    "rc-qs2-mask-hpb2": (1, 2, 30, 9, 64, False, _bw("recompute", 2, True, 2)),
    "rc-qs4": (1, 1, 256, 16, 32, False, _bw("recompute", 4, False, 1)),
    "rc-qs4-mask": (1, 1, 250, 9, 32, False, _bw("recompute", 4, True, 1)),
    "chunk-128x256": (1, 2, 128, 256, 8, False, _bw("chunk", 1, False, 1, bwd_last_chunk_tiles=4)),
    "chunk-dh16": (1, 1, 64, 256, 16, False, _bw("chunk", 1, False, 1)),
    "chunk-mask-120x200": (1, 2, 120, 200, 8, False, _bw("chunk", 1, True, 1, bwd_last_chunk_tiles=1)),
    "swz-256x80": (1, 1, 256, 80, 8, False, _bw("chunk_swz", 1, False, 1, bwd_sc256=False, bwd_last_chunk_tiles=1)),
    "swz-sc256-h1": (1, 1, 256, 256, 8, False, _bw("chunk_swz", 1, False, 1, bwd_sc256=True)),
    "swz-sc256-h8": (1, 8, 256, 256, 8, False, _bw("chunk_swz", 1, False, 1, bwd_sc256=True)),
    "swz-mask-256x77": (1, 2, 256, 77, 8, False, _bw("chunk_swz", 1, True, 1, bwd_last_chunk_tiles=1)),
    "swz-mask-250x256": (1, 2, 250, 256, 8, False, _bw("chunk_swz", 1, True, 1, bwd_last_chunk_tiles=4)),
    "fp8-dh16": (1, 2, 64, 64, 16, True, _bw("lds", 1, False, 1)),
    "fp8-dh32": (1, 2, 64, 64, 32, True, _bw("lds", 1, False, 1)),
    "fp8-dh64": (1, 2, 64, 64, 64, True, _bw("lds", 1, False, 1)),
    "fp8-mask-72x20-dh16": (1, 2, 72, 20, 16, True, _bw("lds", 2, True, 1)),
}


@pytest.mark.parametrize("name", list(BWD))
def test_bwd(O, name):
    """One backward launch per reachable (dS^T mode, QS, MASK, hpb), dq / dk / dv per element, from
    o and lse rounded from the fp64 reference.  Catches: the last unpaired query tile of phase A
    skipped (one sixteenth or more of every dk / dv sum), a QS partial dropped or summed twice, a
    masked query row or key leaking (its P is exp(s - 0)), the swizzled dS^T read with the plain
    pattern or the plain one with the wrong pitch (dq wrong, dk / dv right), a partial last key
    chunk reading the previous chunk's dS^T, head offsets of a multi-head workgroup."""
    B, H, sq, sk, dh, fp8, want = BWD[name]
    expect_plan(A.AttnPlan(B, H, sq, sk, dh, fp8), bwd_rc=A.OK, **want)
    bwd_case(O, randn_inputs(4000 + sq + sk + dh, B, H, sq, sk, dh, fp8), name, 4100 + sq)


CHAINED = {"self-dh8": (1, 2, 80, 80, 8, False), "cross-dh8": (1, 2, 72, 31, 8, False),
           "fp8-dh16": (1, 2, 64, 64, 16, True), "dh64": (1, 2, 64, 64, 64, False)}


@pytest.mark.parametrize("name", list(CHAINED))
def test_chained(O, name):
    """Forward, then the backward on the kernel's OWN o and lse (the real hand-over: o rows with
    their stride, lse [B heads][sq] in natural log); the reference backward is fed those same
    outputs, so only the backward's arithmetic is judged."""
    B, H, sq, sk, dh, fp8 = CHAINED[name]
    c = randn_inputs(5000 + sq + dh, B, H, sq, sk, dh, fp8)
    o, lse, _ = fwd_case(O, c, "chained " + name)
    bwd_case(O, c, "chained " + name, 5100 + sq, own=(o.view, lse.view))


# ====================================================================== refusals, fp32 entries
def test_refusals(O):
    """Shapes the kernels cannot run are refused with the planner's code and nothing is written."""
    from encdiff_amd._lib import HipError
    codes = {A.ERR_SHAPE: "ENCDIFF_ERR_SHAPE", A.ERR_UNSUPPORTED: "ENCDIFF_ERR_UNSUPPORTED"}

    def run(B, H, sq, sk, dh, fp8, bwd, rc):
        p = A.AttnPlan(B, H, sq, sk, dh, fp8)
        assert (p.bwd_rc if bwd else p.fwd_rc) == rc
        c = randn_inputs(6000 + dh, B, H, sq, sk, dh, fp8)
        C = H * dh
        outs = [Guard(B * sq, C, BF16, strided=True), nan_guard(B * H, sq)]
        with pytest.raises(HipError, match=codes[rc]):
            if bwd:
                g = _gen(6001)
                lse = rnd(g, B * H, sq)
                o_in, d_o = rnd(g, B * sq, C, dtype=BF16), rnd(g, B * sq, C, dtype=BF16)
                outs = [Guard(B * sq, C, BF16, strided=True), Guard(B * sk, C, BF16, strided=True),
                        Guard(B * sk, C, BF16, strided=True)]
                O.attention_bwd(c.q, c.k, c.v, o_in, lse, d_o, outs[0].view, outs[1].view, outs[2].view, B, H, sq, sk,
                                dh, fp8=fp8)
            else:
                O.attention_fwd(c.q, c.k, c.v, outs[0].view, outs[1].view, B, H, sq, sk, dh, fp8=fp8)
        torch.cuda.synchronize()
        assert all(R.same_bits(t.buf, t.before) for t in outs), "a refused launch wrote an output"

    for bwd in (False, True):
        run(1, 2, 16, 16, 12, False, bwd, A.ERR_SHAPE)
        run(1, 2, 16, 16, 24, False, bwd, A.ERR_UNSUPPORTED)
    run(1, 1, 64, 64, 128, False, True, A.ERR_UNSUPPORTED)
    run(1, 1, 64, 64, 128, True, False, A.ERR_UNSUPPORTED)
    run(1, 1, 1024, 1024, 64, False, True, A.ERR_SHAPE)   # backward staging alone: 520 KB of LDS


def test_f32(O):
    """ed_attention_fwd_f32 / ed_attention_bwd_f32 (one thread per query or key, 64 per block, keys
    in LDS chunks of 128): masked tails on both sides, two chunks of keys, under the fp32 rule
    against the same restatement.  Catches: threads behind the last query / key storing, the second
    key chunk's offset, D from another row."""
    B, H, sq, sk, dh = 2, 2, 70, 150, 16
    c = randn_inputs(7000, B, H, sq, sk, dh, dtype=F32)
    qs, ks, vs = c.heads()
    r64, r32 = A.attn_fwd(qs, ks, vs, c.scale, dtype=F64), A.attn_fwd(qs, ks, vs, c.scale, dtype=F32)
    o = Guard(B * sq, H * dh, F32, strided=True)
    lse = nan_guard(B * H, sq)
    O.attention_f32(c.q, c.k, c.v, o.view, B, H, sq, sk, dh, lse=lse.view)
    torch.cuda.synchronize()
    o.check()
    lse.check()
    assert_f32_rule(c.split(o.view, sq), r64["o"], r32["o"], "f32 o")
    assert_f32_rule(lse.view.reshape(B * H, sq), r64["lse"], r32["lse"], "f32 lse")
    o_in = place(A.merge_heads(r64["o"], B, sq, H, dh).float(), True)
    lse_in = r64["lse"].float().contiguous()
    d_o = place(rnd(_gen(7001), B * sq, H * dh), True)
    dq = Guard(B * sq, H * dh, F32, strided=True)
    dk, dv = Guard(B * sk, H * dh, F32, strided=True), Guard(B * sk, H * dh, F32, strided=True)
    O.attention_bwd_f32(c.q, c.k, c.v, o_in, lse_in, d_o, dq.view, dk.view, dv.view, B, H, sq, sk, dh)
    torch.cuda.synchronize()
    for t in (dq, dk, dv):
        t.check()
    c.unchanged()
    args = (qs, ks, vs, c.split(o_in, sq), lse_in, c.split(d_o, sq), c.scale)
    b64, b32 = A.attn_bwd(*args, dtype=F64), A.attn_bwd(*args, dtype=F32)
    assert_f32_rule(c.split(dq.view, sq), b64["dq"], b32["dq"], "f32 dq")
    assert_f32_rule(c.split(dk.view, sk), b64["dk"], b32["dk"], "f32 dk")
    assert_f32_rule(c.split(dv.view, sk), b64["dv"], b32["dv"], "f32 dv")
