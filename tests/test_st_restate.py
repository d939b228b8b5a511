"""CPU checks of tests/st_restate.py, the reference of tests/test_gpu_st.py.

With rounding switched off and evaluated in fp64 the chains must be the SpatialTransformer itself.
encdiff_amd/ldm/modules/attention.py's SpatialTransformer / BasicTransformerBlock are parameter
containers (their arithmetic runs inside the HIP executor and calling them raises), so the block is
built from that module -- its parameter names and shapes -- and evaluated by
oracle.encdiff_oracle.spatial_transformer, the repository's CPU statement of attention.py:211-261, on
the module's state_dict; the backward is torch autograd of that evaluation.  Every intermediate
gradient of the restated chains is pinned through the parameter gradient it produces.

Also pinned: the StPlan dispatch table (every reachable (entry, c, tile, waves, MF form) and the ones
that are not) and the n_ctx at which the MFMA key-gradient form ends.
"""
from types import SimpleNamespace

import pytest
import torch

import attn_restate as A
import st_restate as S

F64 = torch.float64
C, TOKENS, B, NCTX, CD = 64, 16, 2, 20, 16


@pytest.fixture(scope="module")
def block():
    from encdiff_amd.ldm.modules.attention import SpatialTransformer
    from oracle import encdiff_oracle as O
    torch.manual_seed(3)
    m = SpatialTransformer(C, 8, C // 8, context_dim=CD).double()
    P = {}
    for n, p in m.state_dict().items():
        scale = 0.1 if n.endswith("bias") else (p.shape[1] ** -0.5 if p.dim() > 1 else 0.1)
        base = 1.0 if (p.dim() == 1 and n.endswith("weight")) else 0.0  # norm gains around 1
        P[n] = (base + scale * torch.randn(p.shape, dtype=F64)).requires_grad_(True)
    x = torch.randn(B, C, 4, 4, dtype=F64, requires_grad=True)
    ctx = torch.randn(B, NCTX, CD, dtype=F64, requires_grad=True)
    dy = torch.randn(B, C, 4, 4, dtype=F64)
    L = SimpleNamespace(heads=8, fp8_min_tokens=0)
    out = O.spatial_transformer(P, "", L, x, ctx)
    out.backward(dy)
    t = "transformer_blocks.0."
    W = {"gn_g": P["norm.weight"], "gn_b": P["norm.bias"], "in": P["proj_in.weight"].reshape(C, C),
         "b_in": P["proj_in.bias"], "g1": P[t + "norm1.weight"], "be1": P[t + "norm1.bias"],
         "qkv": torch.cat([P[t + "attn1.to_q.weight"], P[t + "attn1.to_k.weight"], P[t + "attn1.to_v.weight"]]),
         "out1": P[t + "attn1.to_out.0.weight"], "b_out1": P[t + "attn1.to_out.0.bias"],
         "g2": P[t + "norm2.weight"], "be2": P[t + "norm2.bias"], "q2": P[t + "attn2.to_q.weight"],
         "out2": P[t + "attn2.to_out.0.weight"], "b_out2": P[t + "attn2.to_out.0.bias"],
         "g3": P[t + "norm3.weight"], "be3": P[t + "norm3.bias"],
         "ff1": P[t + "ff.net.0.proj.weight"], "b_ff1": P[t + "ff.net.0.proj.bias"],
         "ff2": P[t + "ff.net.2.weight"], "b_ff2": P[t + "ff.net.2.bias"],
         "po": P["proj_out.weight"].reshape(C, C), "b_po": P["proj_out.bias"]}
    W = {k: v.detach() for k, v in W.items()}
    rows = lambda z: z.detach().permute(0, 2, 3, 1).reshape(B * TOKENS, C)
    return SimpleNamespace(P=P, W=W, t=t, x=rows(x), dy=rows(dy), out=rows(out), ctx=ctx,
                           wk=P[t + "attn2.to_k.weight"].detach(), wv=P[t + "attn2.to_v.weight"].detach())


def _chain(b, tile):
    """forward head, self-attention (attn_restate), forward tail, backward tail, self-attention
    backward, backward head -- rounding off, fp64"""
    W = b.W
    hd = S.head_fwd(b.x, W, B, TOKENS, rounds=False)
    sp = lambda z: A.split_heads(z, B, TOKENS, 8, C // 8)
    q, k, v = (sp(hd.qkv[:, i * C:(i + 1) * C]) for i in range(3))
    scale = (C // 8) ** -0.5
    a1 = A.attn_fwd(q, k, v, scale)
    o1 = A.merge_heads(a1["o"], B, TOKENS, 8, C // 8)
    cr = b.ctx.detach().reshape(B * NCTX, CD)
    k2, v2 = cr @ b.wk.t(), cr @ b.wv.t()
    tl = S.tail_fwd(o1, hd.t0, b.x, k2, v2, W, B, TOKENS, NCTX, rounds=False)
    tb = S.tail_bwd(b.dy, tl, k2, v2, W, B, TOKENS, NCTX, tile, rounds=False)
    g1 = A.attn_bwd(q, k, v, a1["o"], a1["lse"], sp(tb.d_o1), scale)
    d_qkv = torch.cat([A.merge_heads(g1[n], B, TOKENS, 8, C // 8) for n in ("dq", "dk", "dv")], 1)
    hb = S.head_bwd(d_qkv, tb.d_t1, hd.t0, hd.s1, W, tile, rounds=False)
    return SimpleNamespace(hd=hd, o1=o1, tl=tl, tb=tb, hb=hb, d_qkv=d_qkv, k2=k2, v2=v2)


def _close(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= 1e-11 * max(1.0, b.abs().max().item()), f"{what}: {err:.3e}"


def test_forward_is_the_block(block):
    _close(_chain(block, TOKENS).tl.out, block.out, "out")


def test_backward_is_autograd(block):
    b, r = block, _chain(block, TOKENS)
    g = lambda n: b.P[n].grad.reshape(b.P[n].shape[0], -1) if b.P[n].dim() > 1 else b.P[n].grad
    t, tl, tb, hb, hd = b.t, r.tl, r.tb, r.hb, r.hd
    _close(b.dy.t() @ tl.t3, g("proj_out.weight"), "dy")
    _close(tb.d_t3.t() @ tl.a, g(t + "ff.net.2.weight"), "d_t3")
    _close(tb.d_f.t() @ tl.n3, g(t + "ff.net.0.proj.weight"), "d_f")
    _close(tb.ln3[0].sum(0), g(t + "norm3.weight"), "LN3 gamma partials (d_n3)")
    _close(tb.ln3[1].sum(0), g(t + "norm3.bias"), "LN3 beta partials")
    _close(tb.d_t2.t() @ tl.o2, g(t + "attn2.to_out.0.weight"), "d_t2")
    _close(tb.d_q2.t() @ tl.n2, g(t + "attn2.to_q.weight"), "d_q2")
    dkv = tb.dkv.reshape(B * NCTX, 2 * C)
    _close((dkv[:, :C] @ b.wk + dkv[:, C:] @ b.wv).reshape(B, NCTX, CD), b.ctx.grad, "dK2 / dV2")
    _close(tb.ln2[0].sum(0), g(t + "norm2.weight"), "LN2 gamma partials (d_n2)")
    _close(tb.ln2[1].sum(0), g(t + "norm2.bias"), "LN2 beta partials")
    _close(tb.d_t1.t() @ r.o1, g(t + "attn1.to_out.0.weight"), "d_t1")
    _close(r.d_qkv[:, :C].t() @ hd.n1, g(t + "attn1.to_q.weight"), "d_o1 (through the self-attention)")
    _close(hb.ln1[0].sum(0), g(t + "norm1.weight"), "LN1 gamma partials (d_n1)")
    _close(hb.ln1[1].sum(0), g(t + "norm1.bias"), "LN1 beta partials")
    _close(hb.d_t0.t() @ hd.gn, g("proj_in.weight"), "d_t0")
    _close(hb.d_gn.sum(0), g("norm.bias"), "d_gn")
    xh = (hd.gn - b.W["gn_b"]) / b.W["gn_g"]
    _close((hb.d_gn * xh).sum(0), g("norm.weight"), "d_gn (gamma)")


def test_tiles_partition_the_sums(block):
    """Per-tile LayerNorm partial rows and dK | dV slabs (two 8-row tiles per image) add up to the
    one-tile results, and kv_fold is the in-order fp32 sum rounded once."""
    one, two = _chain(block, TOKENS).tb, _chain(block, TOKENS // 2).tb
    assert two.ln3[0].shape == (2 * B, C) and two.dkv.shape == (2 * B, NCTX, 2 * C)
    for a, b_ in zip(one.ln3 + one.ln2, two.ln3 + two.ln2):
        _close(b_.reshape(B, 2, C).sum(1), a, "partial rows")
    _close(two.dkv.reshape(B, 2, NCTX, 2 * C).sum(1), one.dkv, "slabs")
    s32 = two.dkv.float()
    fold = S.kv_fold(s32, 2)
    want = (s32.reshape(B, 2, NCTX, 2 * C)[:, 0] + s32.reshape(B, 2, NCTX, 2 * C)[:, 1]).reshape(B * NCTX, 2 * C)
    assert torch.equal(fold.view(torch.int16), want.bfloat16().view(torch.int16))


def test_gn_sums_forms_agree():
    torch.manual_seed(1)
    x = torch.randn(2 * 128, 64, dtype=F64) + 0.3
    a = S.gn_stats_from_sums(S.gn_sums(x), 2, 128, 64, 1e-6)
    b = S.gn_stats_from_x(x, 2, 128, 64, 1e-6)
    assert (a - b).abs().max().item() < 1e-12
    g, be = torch.randn(64, dtype=F64), torch.randn(64, dtype=F64)
    want = torch.nn.functional.group_norm(x.reshape(2, 128, 64).transpose(1, 2), 32, g, be, 1e-6).transpose(1, 2)
    assert (S.gn_apply(x, a, g, be, 2, 128) - want.reshape(256, 64)).abs().max().item() < 1e-10


def test_half_ulp():
    v = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 0.0, -3.0], dtype=F64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0, 2.0 ** -7], dtype=F64)
    assert torch.equal(S.half_ulp(v), want)
    x = torch.randn(4096, dtype=F64) * 3
    assert ((x.bfloat16().double() - x).abs() <= S.half_ulp(x)).all()
    assert (S.half_ulp(x) >= 2.0 ** -9 * x.abs()).all() and (S.half_ulp(x) <= 2.0 ** -8 * x.abs()).all()
    # why the store term is the half-ulp and not a flat 2^-9 |v|: a CORRECT rounding exceeds the flat
    # figure for about a quarter of all values (those in the lower part of their binade)
    assert ((x.bfloat16().double() - x).abs() > 2.0 ** -9 * x.abs()).double().mean().item() > 0.2


# ---------------------------------------------------------------------------- dispatch
def test_mf_boundaries():
    """The MFMA key-gradient form ends where TailBwd::lds_bytes(n_ctx, MF) passes 80 KiB (two
    workgroups per CU), 160 KiB for the c = 128 64-row tile; worked from the formula:
      c 64 / 64 rows:  45136 + 256 n + 1024 jp(n) <= 81920   -> n <= 28 (80976; n = 29: jp 32, 85328)
      c 128 / 32 rows: 43088 + 512 n + 1024 jp(n) <= 81920   -> n <= 24 (79952; n = 25: jp 28, 84560)
      c 128 / 64 rows: 86096 + 512 n + 1024 jp(n) <= 163840  -> n <= 48 (159824; n = 49: jp 52, 164432)"""
    assert S.tail_bwd_lds(64, 64, 28, True) == 80976 and S.tail_bwd_lds(64, 64, 29, True) == 85328
    assert S.tail_bwd_lds(128, 32, 24, True) == 79952 and S.tail_bwd_lds(128, 32, 25, True) == 84560
    assert S.tail_bwd_lds(128, 64, 48, True) == 159824 and S.tail_bwd_lds(128, 64, 49, True) == 164432
    assert (S.mf_last(64, 64), S.mf_last(128, 32), S.mf_last(128, 64)) == (28, 24, 48)
    # the VALU form always fits at n_ctx = 64
    assert max(S.tail_bwd_lds(c, R, 64, False) for c, R in ((64, 64), (128, 32), (128, 64))) <= S.LDS_MAX
    for c, R, last in ((64, 64, 28), (128, 32, 24)):
        rows = 128
        assert S.StPlan.tail_bwd(c, rows, 64, last).mf and not S.StPlan.tail_bwd(c, rows, 64, last + 1).mf
    assert S.StPlan.tail_bwd(128, 16384, 64, 48).mf and not S.StPlan.tail_bwd(128, 16384, 64, 49).mf


def test_plan_table():
    """Every (entry, c, tile, waves, MF) the dispatch reaches.  NOT reachable: the c = 64 tail on 32
    rows without ENCDIFF_ST_TAIL_R32_C64 (listed here because the add form's flag reaches it), a 64-row
    tile at c = 256, the c = 64 head on 32 rows (ED_HEAD64_R32 off), the c = 256 head on 32 / 64 rows
    or with 4 waves, any backward at c = 256, the c = 128 head backward on 64 rows."""
    want = {("tail_fwd", 64, 16, 4, None), ("tail_fwd", 64, 32, 4, None), ("tail_fwd", 64, 64, 4, None),
            ("tail_fwd", 128, 16, 8, None), ("tail_fwd", 128, 16, 4, None), ("tail_fwd", 128, 32, 8, None),
            ("tail_fwd", 128, 32, 4, None), ("tail_fwd", 128, 64, 8, None), ("tail_fwd", 128, 64, 4, None),
            ("tail_fwd", 256, 16, 4, None), ("tail_fwd", 256, 16, 8, None), ("tail_fwd", 256, 32, 4, None),
            ("head_fwd", 64, 16, 4, None), ("head_fwd", 64, 64, 4, None), ("head_fwd", 128, 16, 4, None),
            ("head_fwd", 128, 32, 4, None), ("head_fwd", 128, 64, 4, None), ("head_fwd", 256, 16, 8, None),
            ("tail_bwd", 64, 64, 4, True), ("tail_bwd", 64, 64, 4, False), ("tail_bwd", 128, 32, 4, True),
            ("tail_bwd", 128, 32, 4, False), ("tail_bwd", 128, 64, 4, True), ("tail_bwd", 128, 64, 4, False),
            ("head_bwd", 64, 32, 4, None), ("head_bwd", 64, 64, 4, None), ("head_bwd", 128, 32, 4, None)}
    assert S.reachable() == want


def test_plan_cases():
    P = S.StPlan
    # forward tail: thresholds, images per tile, key-split lanes, the LDS fallback, statistics forms
    p = P.tail_fwd(64, 32, 4, 20)
    assert (p.tile, p.waves, p.nimg, p.spl, p.grid) == (16, 4, 4, 2, 2)
    assert P.tail_fwd(128, 16, 4, 20).spl == 4 and P.tail_fwd(64, 16384, 256, 20).spl == 1
    assert P.tail_fwd(64, 16368, 16, 20).tile == 16 and P.tail_fwd(64, 16384, 256, 20).tile == 64
    assert P.tail_fwd(64, 16384, 4, 40).tile == 16      # 16 images' K / V do not fit: 64 rows declined
    assert P.tail_fwd(64, 16384, 4, 20).tile == 64
    assert P.tail_fwd(256, 8192, 16, 20).tile == 32 and P.tail_fwd(256, 4096, 16, 20).tile == 16
    assert P.tail_fwd(256, 4096, 16, 20, head=True).waves == 4 and P.tail_fwd(256, 4080, 16, 20, head=True).waves == 8
    assert P.tail_fwd(128, 128, 64, 20, gn_stats=True, add=P.stats_add(128, 128)).key() == ("tail_fwd", 128, 32, 8, None)
    assert P.tail_fwd(128, 8192, 64, 20, gn_stats=True, add=True).waves == 4
    assert P.tail_fwd(128, 16384, 64, 20, gn_stats=True, add=P.stats_add(128, 16384)).tile == 64
    assert not P.stats_add(64, 128) and P.stats_add(64, 128, r32_c64=True) and not P.stats_add(128, 128, stats_add=False)
    assert P.tail_fwd(256, 64, 16, 20, gn_stats=True).rc == S.ERR_SHAPE
    assert P.tail_fwd(64, 96, 16, 20, gn_stats=True).rc == S.ERR_SHAPE
    assert P.tail_fwd(64, 128, 16, 65).rc == S.ERR_SHAPE and P.tail_fwd(32, 128, 16, 20).rc == S.ERR_UNSUPPORTED
    # forward head
    assert P.head_fwd(64, 128, 64).tile == 16 and P.head_fwd(64, 16384, 256).tile == 64
    assert P.head_fwd(128, 8192, 64).tile == 32 and P.head_fwd(128, 8160, 32).tile == 16
    assert P.head_fwd(256, 32, 16).waves == 8 and P.head_fwd(256, 32, 16, n1=True).rc == S.ERR_SHAPE
    assert P.head_fwd(256, 4096, 16).rc == S.ERR_SHAPE and P.head_fwd(64, 8, 4).rc == S.ERR_SHAPE
    assert P.head_fwd(64, 32, 16, in_stats=True).rc == S.ERR_SHAPE
    # backward
    assert P.tail_bwd_tile(128, 16384, 64) == 64 and P.tail_bwd_tile(128, 16384, 32) == 32
    assert P.tail_bwd(64, 32, 16, 20).rc == S.ERR_SHAPE and P.tail_bwd(256, 64, 64, 20).rc == S.ERR_UNSUPPORTED
    assert P.tail_bwd(64, 256, 256, 20, part_rows=3).rc == S.ERR_SHAPE and P.tail_bwd(64, 256, 256, 20).tpi == 4
    assert P.head_bwd(64, 16384).tile == 64 and P.head_bwd(64, 16352).tile == 32 and P.head_bwd(128, 16384).tile == 32
    assert P.head_bwd(64, 48).rc == S.ERR_SHAPE


def test_plan_refuses_knobs(monkeypatch):
    for k in S.KNOBS:
        monkeypatch.setenv(k, "1")
        with pytest.raises(AssertionError):
            S.StPlan.head_bwd(64, 64)
        monkeypatch.delenv(k)
