"""CPU checks of tests/attn_restate.py, the references of tests/test_gpu_attention.py: the forward
and backward restatements are held against torch's fp64 autograd of plain softmax attention, the
fp8 variant against the formulation of test_gpu_ops.py::test_attention_fp8_scores, and the copy of
the launch planner against shapes worked by hand from launch_mfma_fwd / launch_mfma_bwd."""
import pytest
import torch

import attn_restate as A

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _close(a, b, tol=1e-11):
    scale = max(1.0, b.abs().max().item())
    assert (a - b).abs().max().item() <= tol * scale, (a - b).abs().max().item()


def _inputs(B, H, sq, sk, dh, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda s: torch.randn(B * H, s, dh, generator=g).to(BF16)
    return mk(sq), mk(sk), mk(sk), mk(sq)


@pytest.mark.parametrize("B,H,sq,sk,dh", [(2, 3, 37, 21, 8), (1, 2, 32, 32, 16)], ids=["masked-tail", "square"])
def test_restatement_matches_autograd(B, H, sq, sk, dh):
    """o, lse and the three gradients against autograd of softmax(q k^T scale) v in fp64.  The
    backward restatement is fed the exact fp64 o and lse here, so it must reproduce autograd: a
    transposed dS, a missing scale, D taken from the wrong tensor or an LSE in the log2 domain shows."""
    q, k, v, d_o = _inputs(B, H, sq, sk, dh, sq + dh)
    scale = dh ** -0.5
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qr @ kr.transpose(1, 2) * scale
    o = s.softmax(-1) @ vr
    o.backward(d_o.double())
    f = A.attn_fwd(q, k, v, scale)
    _close(f["o"], o.detach())
    _close(f["lse"], torch.logsumexp(s.detach(), -1))
    _close(f["abs_o"], s.detach().softmax(-1) @ v.double().abs())
    assert (f["abs_o"] >= f["o"].abs() - 1e-12).all()
    b = A.attn_bwd(q, k, v, f["o"], f["lse"], d_o, scale)
    _close(b["dq"], qr.grad)
    _close(b["dk"], kr.grad)
    _close(b["dv"], vr.grad)
    for n in ("dq", "dk", "dv"):
        assert (b["abs_" + n] >= b[n].abs() - 1e-12).all()
    # the backward uses ITS givens: a shifted lse scales P, a changed o moves D
    b2 = A.attn_bwd(q, k, v, f["o"], f["lse"] + 1.0, d_o, scale)
    _close(b2["dv"], vr.grad * torch.exp(torch.tensor(-1.0, dtype=F64)))
    # rows layout round trip
    rows = A.merge_heads(f["o"], B, sq, H, dh)
    assert rows.shape == (B * sq, H * dh)
    assert torch.equal(A.split_heads(rows, B, sq, H, dh), f["o"])
    b_, h_ = B - 1, H - 1  # image b_, head h_, query 3 sits in row b_ sq + 3, columns h_ dh ..
    assert torch.equal(rows[b_ * sq + 3, h_ * dh:(h_ + 1) * dh], f["o"][b_ * H + h_, 3])


def test_fp8_restatement_matches_the_existing_formulation():
    """fp8: scores from q, k rounded to float8_e4m3fn, every gradient product from the bf16 q, k --
    the formulation of test_attention_fp8_scores, here in fp64."""
    B, H, sq, sk, dh = 2, 2, 24, 20, 16
    q, k, v, d_o = _inputs(B, H, sq, sk, dh, 3)
    scale = dh ** -0.5
    e4 = torch.float8_e4m3fn
    qs, ks, vs, gs = q.double(), k.double(), v.double(), d_o.double()
    att = (q.to(e4).double() @ k.to(e4).double().transpose(1, 2) * scale).softmax(-1)
    ref = att @ vs
    dp = gs @ vs.transpose(1, 2)
    dsc = att * (dp - (dp * att).sum(-1, keepdim=True))
    f = A.attn_fwd(q, k, v, scale, fp8=True)
    _close(f["o"], ref)
    b = A.attn_bwd(q, k, v, f["o"], f["lse"], d_o, scale, fp8=True)
    _close(b["dq"], dsc @ ks * scale)
    _close(b["dk"], dsc.transpose(1, 2) @ qs * scale)
    _close(b["dv"], att.transpose(1, 2) @ gs)
    assert (A.attn_fwd(q, k, v, scale)["o"] - f["o"]).abs().max() > 1e-4  # the rounding is really applied


def test_row_bounds():
    """sqrt(|q|^2 max|k|^2) scale log2e 1.001 + 1e-6 by hand, and the per-task verdict."""
    q = torch.zeros(1, 40, 16)
    q[0, :, 0] = 3.0
    q[0, 17, 0] = 300.0
    k = torch.zeros(1, 5, 16)
    k[0, 2, 1] = 4.0
    b = A.row_bounds(q.to(BF16), k.to(BF16), 0.25)
    assert abs(b[0, 0].item() - (12 * 0.25 * A.LOG2E * 1.001 + 1e-6)) < 1e-5
    assert b[0, 17].item() > 40
    assert A.task_on_bound_path(b, 2).tolist() == [[False, True]]   # rows 0..31 | 32..39
    assert A.task_on_bound_path(b, 4).tolist() == [[False]]


def test_fp8_lse_slack_by_hand():
    """One key, dh 8 (one group of 8 products): 16 x 16 = 2^8 sets the granularity 2^-5; 2^-6 x 1 is no
    multiple of it and may be lost whole, 2^-3 x 1 is kept.  With one key lse = s, so the slack is D."""
    q = torch.zeros(1, 3, 8)
    k = torch.zeros(1, 1, 8)
    q[0, :, 0], k[0, 0, 0], k[0, 0, 1] = 16.0, 16.0, 1.0
    q[0, 1, 1] = 2.0 ** -6
    q[0, 2, 1] = 2.0 ** -3
    got = A.fp8_lse_slack(q.to(BF16), k.to(BF16), 0.5)
    assert got.shape == (1, 3)
    assert torch.allclose(got[0], torch.tensor([0.0, 2.0 ** -5 * 0.5, 0.0], dtype=F64), rtol=0, atol=1e-12)


def test_dv_p_slack_between_half_and_whole_bf16_rounding():
    q, k, v, d_o = _inputs(1, 2, 16, 90, 16, 9)
    f = A.attn_fwd(q, k, v, 0.25)
    b = A.attn_bwd(q, k, v, f["o"], f["lse"], d_o, 0.25)
    s = A.dv_p_slack(b)
    assert (s >= 2.0 ** -9 * b["abs_dv"]).all() and (s <= 2.0 ** -8 * b["abs_dv"] * (1 + 1e-12)).all()
    assert (b["round_dv"] > 2.0 ** -9 * b["abs_dv"]).any()   # few queries: some columns do not average


def plan(*a, **kw):
    return A.AttnPlan(*a, **kw)


def has(p, **want):
    for k, v in want.items():
        assert getattr(p, k) == v, f"{k} = {getattr(p, k)}, expected {v}"


def test_planner_forward_by_hand():
    # hpb: 4 heads per workgroup below 64 queries, halved until it divides the head count
    has(plan(1, 4, 4, 4, 32), fwd_hpb=4, fwd_mask=True, fwd_npairs=1, fwd_grid=(1, 1), fwd_lds=4 * 2 * 32 * 32 * 2 + 64)
    has(plan(2, 4, 48, 40, 16), fwd_hpb=4, fwd_npairs=2, fwd_grid=(2, 1), fwd_mask=True, fwd_bound_eligible=True)
    has(plan(1, 2, 16, 20, 8), fwd_hpb=2, fwd_lds=2 * 2 * 32 * 16 * 2 + 64)          # dh 8 padded to 16
    has(plan(1, 3, 16, 33, 16), fwd_hpb=1, fwd_kch=64, fwd_grid=(3, 1))
    has(plan(1, 8, 64, 64, 16), fwd_hpb=1, fwd_mask=False)
    # dh 8: four 16-query tiles per task; sq 72 = 5 tiles -> 2 tasks, 3 tiles of the second invalid
    has(plan(1, 1, 72, 31, 8), fwd_npairs=2, fwd_mask=True, fwd_idle_waves=2)
    has(plan(1, 1, 80, 32, 8), fwd_npairs=2, fwd_mask=False)
    has(plan(1, 1, 80, 33, 8), fwd_kch=64, fwd_mask=True)
    # SC256 only at dh 8, bf16 scores, 256 x 256
    has(plan(1, 1, 256, 256, 8), fwd_sc256=True, fwd_mask=False, fwd_grid=(1, 1))
    has(plan(1, 8, 256, 256, 8), fwd_sc256=True, fwd_grid=(8, 1))
    has(plan(1, 8, 256, 256, 8, fp8=True), fwd_sc256=False, fwd_bound_eligible=False)
    has(plan(1, 1, 256, 256, 16), fwd_sc256=False)
    # wide single heads: query tasks over blockIdx.y while 2 nqb nx <= 256 and npairs >= 8 nqb
    has(plan(2, 1, 256, 256, 128), fwd_nqb=2, fwd_npairs=8, fwd_streamed=False, fwd_lds=2 * 256 * 128 * 2 + 64,
        fwd_idle_waves=0, fwd_bound_eligible=False)
    has(plan(2, 1, 256, 256, 64), fwd_nqb=2, fwd_streamed=False)
    has(plan(2, 1, 272, 272, 128), fwd_nqb=2, fwd_npairs=9, fwd_mask=True, fwd_idle_waves=7, fwd_lds=2 * 288 * 128 * 2 + 64)
    has(plan(4, 8, 64, 64, 64), fwd_nqb=1)
    # K / V beyond 160 KB: one head, 64 KB chunks (dh 128: 128 keys; dh 64: 256; dh 8 / 16: 1024)
    has(plan(1, 1, 1000, 1000, 128), fwd_streamed=True, fwd_kch=128, fwd_nqb=8, fwd_npairs=32, fwd_last_chunk=128,
        fwd_mask=True, fwd_lds=65536 + 64)
    has(plan(1, 1, 1048, 1048, 128), fwd_streamed=True, fwd_nqb=9, fwd_last_chunk=32, fwd_idle_waves=3)
    has(plan(1, 1, 40, 650, 64), fwd_streamed=True, fwd_kch=256, fwd_nqb=1, fwd_last_chunk=160, fwd_idle_waves=2)
    has(plan(1, 4, 16, 1100, 8), fwd_hpb_fallback=True, fwd_hpb=1, fwd_streamed=True, fwd_kch=1024, fwd_last_chunk=96,
        fwd_grid=(4, 1))
    has(plan(2, 1, 1024, 1024, 128), fwd_streamed=True, fwd_nqb=8)
    has(plan(1, 1, 1024, 1024, 16), fwd_streamed=False, fwd_hpb_fallback=False, fwd_lds=65536 + 64)
    # the fallback with exactly kch padded keys stays RESIDENT: the key norms sit behind K / V and
    # the allocation has to hold them
    for shape in [(1, 4, 16, 1024, 8), (1, 4, 16, 1000, 16), (1, 4, 16, 993, 8), (1, 4, 16, 512, 32), (1, 4, 16, 481, 32)]:
        p = plan(*shape)
        has(p, fwd_hpb_fallback=True, fwd_hpb=1, fwd_streamed=False, fwd_bound_eligible=True, fwd_lds_used=65536 + 4)
        assert p.fwd_lds >= p.fwd_lds_used
    # one tile of keys fewer: still the fallback (4 heads of 640 .. 992 padded keys exceed 160 KB), kn inside
    has(plan(1, 4, 16, 992, 8), fwd_hpb_fallback=True, fwd_hpb=1, fwd_streamed=False, fwd_lds_used=2 * 992 * 16 * 2 + 4)
    has(plan(1, 4, 16, 608, 8), fwd_hpb_fallback=False, fwd_hpb=4, fwd_lds=4 * 2 * 608 * 16 * 2 + 64)
    has(plan(1, 4, 16, 1025, 8), fwd_streamed=True)
    has(plan(1, 4, 16, 480, 32), fwd_hpb_fallback=True, fwd_streamed=False, fwd_lds_used=2 * 480 * 32 * 2 + 4)
    has(plan(1, 4, 16, 288, 32), fwd_hpb_fallback=False, fwd_hpb=4)
    # fp8 shapes
    has(plan(1, 2, 72, 20, 16, fp8=True), fwd_mask=True, fwd_bound_eligible=False, fwd_hpb=1)


def test_planner_lds_covers_every_shape():
    """The forward allocation holds what the kernel addresses (K, V of the resident rows and, on the
    resident branch, the key norms behind them) for every sk up to 1200 at every head dim."""
    for dh in (8, 16, 32, 64, 128):
        for heads, sq in ((4, 16), (2, 16), (1, 16), (1, 64)):
            for sk in range(1, 1201):
                p = plan(1, heads, sq, sk, dh)
                assert p.fwd_rc == A.OK
                assert p.fwd_lds_used <= p.fwd_lds <= A.LDS_MAX, (dh, heads, sq, sk, p.fwd_lds_used, p.fwd_lds)


def test_planner_backward_by_hand():
    # QS: 4 / 2 / 1 for ktiles x hpb = 1 / 2..3 / >= 4
    has(plan(1, 1, 64, 16, 8), bwd_mode="lds", bwd_qs=4, bwd_mask=False, bwd_hpb=1, bwd_loop_even=False,
        bwd_lds=(128 + 32) * 8 * 2 + 2 * 64 * 4 + 4 * 2 * 16 * 16 * 4 + 16 * 80 * 2)
    has(plan(1, 1, 64, 9, 32), bwd_mode="lds", bwd_qs=4, bwd_mask=True)
    has(plan(1, 1, 128, 16, 8), bwd_mode="lds", bwd_qs=4, bwd_loop_even=True)
    has(plan(1, 1, 64, 20, 8), bwd_mode="lds", bwd_qs=2, bwd_mask=True, bwd_loop_even=True)
    has(plan(1, 3, 16, 33, 16), bwd_mode="lds", bwd_qs=2, bwd_hpb=1, bwd_loop_even=False)
    has(plan(1, 4, 4, 4, 32), bwd_mode="lds", bwd_qs=1, bwd_hpb=4, bwd_mask=True)
    has(plan(1, 4, 48, 40, 16), bwd_mode="lds", bwd_qs=1, bwd_hpb=4, bwd_lds=50688)
    has(plan(1, 2, 16, 20, 8), bwd_mode="lds", bwd_qs=1, bwd_hpb=2, bwd_mask=True)
    has(plan(1, 2, 16, 16, 8), bwd_mode="lds", bwd_qs=2, bwd_hpb=2, bwd_mask=False)
    has(plan(1, 1, 64, 64, 64), bwd_mode="lds", bwd_qs=1, bwd_lds=43520)
    # recompute: base + dS^T above 52 KB and no chunking (hpb > 1, QS > 1, sq > 256 or base too large)
    has(plan(1, 1, 512, 20, 8), bwd_mode="recompute", bwd_qs=2, bwd_mask=True, bwd_loop_even=True)
    has(plan(1, 4, 48, 256, 16), bwd_mode="recompute", bwd_qs=1, bwd_hpb=4, bwd_mask=False)
    has(plan(1, 1, 1024, 1024, 16), bwd_mode="recompute", bwd_qs=1, bwd_lds=139264)
    has(plan(1, 1, 1024, 1024, 16, fp8=True), bwd_mode="recompute")
    has(plan(1, 1, 16, 40, 64), bwd_mode="recompute", bwd_qs=2, bwd_mask=True)
    has(plan(1, 1, 256, 16, 32), bwd_mode="recompute", bwd_qs=4)
    # 256 x 256 at dh 16 does NOT chunk: base 34816 + chunk 34816 > 56 KB
    has(plan(1, 1, 256, 256, 16), bwd_mode="recompute", bwd_lds=34816)
    has(plan(1, 1, 250, 256, 16), bwd_mode="recompute", bwd_mask=True)
    # chunked dS^T (64 keys): plain pitch below 256 padded queries, swizzled at 256
    has(plan(1, 1, 128, 256, 8), bwd_mode="chunk", bwd_dsl=64, bwd_mask=False, bwd_last_chunk_tiles=4,
        bwd_lds=(256 + 512) * 8 * 2 + 1024 + 64 * 144 * 2)
    has(plan(1, 1, 120, 200, 8), bwd_mode="chunk", bwd_mask=True, bwd_last_chunk_tiles=1)
    has(plan(1, 1, 64, 256, 16), bwd_mode="chunk", bwd_mask=False)
    has(plan(1, 1, 256, 256, 8), bwd_mode="chunk_swz", bwd_sc256=True, bwd_mask=False, bwd_lds=53248)
    has(plan(1, 8, 256, 256, 8), bwd_mode="chunk_swz", bwd_sc256=True)
    has(plan(1, 1, 256, 77, 8), bwd_mode="chunk_swz", bwd_sc256=False, bwd_mask=True, bwd_last_chunk_tiles=1)
    has(plan(1, 1, 250, 256, 8), bwd_mode="chunk_swz", bwd_sc256=False, bwd_mask=True, bwd_last_chunk_tiles=4)
    has(plan(1, 1, 256, 80, 8), bwd_mode="chunk_swz", bwd_mask=False)
    has(plan(1, 8, 256, 256, 8, fp8=True), bwd_mode="chunk_swz", bwd_sc256=False)


def test_planner_refusals():
    assert plan(1, 2, 16, 16, 12).fwd_rc == A.ERR_SHAPE and plan(1, 2, 16, 16, 12).bwd_rc == A.ERR_SHAPE
    assert plan(1, 2, 16, 16, 24).fwd_rc == A.ERR_UNSUPPORTED
    assert plan(1, 1, 64, 64, 128).fwd_rc == A.OK and plan(1, 1, 64, 64, 128).bwd_rc == A.ERR_UNSUPPORTED
    assert plan(1, 1, 64, 64, 128, fp8=True).fwd_rc == A.ERR_UNSUPPORTED
    p = plan(1, 1, 1024, 1024, 64)
    assert p.fwd_rc == A.OK and p.bwd_rc == A.ERR_SHAPE and p.bwd_lds == 532480
    assert plan(1, 1, 40, 650, 64).bwd_rc == A.ERR_SHAPE
    assert plan(0, 1, 4, 4, 8).fwd_rc == A.ERR_SHAPE


def test_reachable_backward_combinations():
    """The (mode, QS, MASK, hpb) combinations the planner can produce for sq, sk <= 1024: the list
    tests/test_gpu_attention.py covers case by case.  The chunked modes exist only with hpb 1 and
    QS 1, QS 4 only with hpb 1, QS 2 never with hpb 4."""
    r = set(A.reachable_bwd())
    want = {("lds", 1, m, h) for m in (False, True) for h in (1, 2, 4)}
    want |= {("lds", 2, m, h) for m in (False, True) for h in (1, 2)}
    want |= {("lds", 4, m, 1) for m in (False, True)}
    want |= {("recompute", 1, m, h) for m in (False, True) for h in (1, 2, 4)}
    want |= {("recompute", 2, m, h) for m in (False, True) for h in (1, 2)}
    want |= {("recompute", 4, m, 1) for m in (False, True)}
    want |= {(c, 1, m, 1) for c in ("chunk", "chunk_swz") for m in (False, True)}
    assert r == want
