"""CPU checks of tests/gemm_fused_restate.py, the restatement tests/test_gpu_gemm_fused.py holds the
GEMM's fused norm and GEGLU stagings and epilogues to.

1. The stages in fp64 against torch: F.group_norm / F.silu + F.conv2d (F.interpolate nearest for UP2),
   F.layer_norm + matmul, F.gelu (erf) and its autograd.
2. The enum values against encdiff_amd._lib; the three findings test_gpu_gemm_fused.py's docstring lists,
   as far as the host validation (encdiff_gemm_check, no launch) shows them.
3. The bounds are sharp, on the very inputs the GPU cases use (the case tables of the restatement):
   a model of each kernel (fp32 one-pass statistics in the kernel's order, the operand rounded to bf16,
   fp32 accumulation, a bf16 store) stays inside the bound, and every listed mutation exceeds it on at
   least half of the output elements of at least one case.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import gemm_fused_restate as FR
import gemm_restate as G
import st_restate as S

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def strided(kind, t):
    """2-D operands as column views of wider NaN-padded buffers, as the GPU cases place them"""
    if t.dim() != 2:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + 24), float("nan"), dtype=t.dtype)
    buf[:, 8:8 + t.shape[1]] = t
    return buf[:, 8:8 + t.shape[1]]


# ====================================================================== 1. the stages against torch
@pytest.mark.parametrize("name", ["b3-2x2-c32", "b2-8x8-c96", "b5-3x5-c32", "b8-up4x4-c64", "b2-up16x16-c32",
                                  "b20-1x1-c64", "b1-8x8-c64"])
def test_agn_is_groupnorm_film_silu_conv(name):
    I = FR.agn_inputs(name, strided)
    c = I.case
    B, cin, cout = I.B, I.cin, I.cout
    hs, ws = (I.hh // 2, I.ww // 2) if c["up2"] else (I.hh, I.ww)
    x = I.x.double().reshape(B, hs, ws, cin).permute(0, 3, 1, 2)
    n = F.group_norm(x, 32, I.gamma.double(), I.beta.double(), I.eps)
    if I.film is not None:
        sc, sh = I.film[:, :cin].double(), I.film[:, cin:2 * cin].double()
        n = n * (1 + sc[:, :, None, None]) + sh[:, :, None, None]
    if I.silu:
        n = F.silu(n)
    if c["up2"]:
        n = F.interpolate(n, scale_factor=2, mode="nearest")
    w = I.w.double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)   # packed [cout][tap][cin]
    y = F.conv2d(n, w, None if I.bias is None else I.bias.double(), padding=1)
    y = y.permute(0, 2, 3, 1).reshape(I.M, cout)
    if I.resid is not None:
        y = y + I.resid.double()
    h, _ = FR.agn_act(I.x, B, I.shw, I.gamma, I.beta, I.film, I.eps, I.silu, F64)
    got = FR.linear_out(FR.with_a(I.P, h), F64)
    assert (got - y).abs().max().item() < 1e-11


@pytest.mark.parametrize("name", list(FR.LNA_CASES))
def test_lna_is_layernorm_linear(name):
    I = FR.lna_inputs(name, strided)
    n = F.layer_norm(I.x.double(), (I.K,), I.gamma.double(), I.beta.double(), I.eps)
    y = n @ I.w.double().t()
    if I.bias is not None:
        y = y + I.bias.double()
    if I.resid is not None:
        y = y + I.resid.double()
    got = FR.linear_out(FR.with_a(I.P, FR.lna_act(I.x, I.gamma, I.beta, I.eps, F64)), F64)
    assert (got - y).abs().max().item() < 1e-11


def test_ln_y_is_layernorm():
    I = FR.lny_inputs("t4-m65-n64", strided)
    c = FR.linear_out(I.P, F64).to(BF16)
    y, st = FR.ln_y_stage(c, I.gamma, I.beta, I.eps, F64)
    ref = F.layer_norm(c.double(), (I.N,), I.gamma.double(), I.beta.double(), I.eps)
    assert (y - ref).abs().max().item() < 1e-12
    assert torch.allclose(st[:, 0], c.double().mean(1), atol=1e-14)
    assert torch.allclose(st[:, 1], 1 / torch.sqrt(c.double().var(1, unbiased=False) + I.eps), rtol=1e-13)


def test_geglu_is_gelu_and_its_autograd():
    I = FR.geglu_bwd_inputs("t4-m130-n200", strided)
    f = I.f.double()
    i = I.N
    a, g = f[:, :i].clone().requires_grad_(True), f[:, i:].clone().requires_grad_(True)
    y = a * F.gelu(g)
    assert (FR.geglu_y(I.f, F64) - y.detach()).abs().max().item() < 1e-13
    d = FR.linear_out(I.P, F64)
    assert (d - I.dy.double() @ I.w.double()).abs().max().item() < 1e-12
    y.backward(d)
    ref = torch.cat([a.grad, g.grad], 1)
    assert (FR.geglu_bwd(d, I.f, F64) - ref).abs().max().item() < 1e-11


def test_geglu_forward_is_chunked_linear():
    I = FR.geglu_inputs("t4-m130-n256", strided)
    f = F.linear(I.x.double(), I.w.double()) * I.alpha
    assert I.bias is None
    assert (FR.linear_out(I.P, F64) - f).abs().max().item() < 1e-12
    v, gate = f.chunk(2, dim=-1)
    assert (FR.geglu_y(f, F64) - v * F.gelu(gate)).abs().max().item() < 1e-13


# ====================================================================== 2. the binding and the host validation
def test_enums_match_the_binding():
    import encdiff_amd._lib as L
    assert (L.OUT_BF16_GEGLU, L.OUT_BF16_GEGLU_BWD) == (FR.OUT_BF16_GEGLU, FR.OUT_BF16_GEGLU_BWD)
    assert L.RESAMPLE_UP2 == G.UP2 and L.OUT_BF16 == G.OUT_BF16
    assert set(FR.FUSED_ROUNDS) >= {"agn_h", "lna_h", "ln_y", "geglu_y", "geglu_d"}


A16 = 1 << 12   # a fake, 16-byte aligned address: encdiff_gemm_check reads no operand


def check(**kw):
    import encdiff_amd._lib as L
    conv = kw.pop("conv", None)
    cg = L.ConvGeom() if conv is None else L.ConvGeom(batch=conv[0], h=conv[1], w=conv[2], cin=conv[3],
                                                      resample=conv[4], ld_src=conv[3])
    base = dict(a_mode=0, b_mode=0, c_mode=0, a=A16, b=A16, c=A16, alpha=1.0, split_k=1, tile=4, conv=cg)
    base.update(kw)
    args = L.GemmArgs(**base)
    return L.lib.encdiff_gemm_check(C.byref(args), None)


def agn_check(B, h, w, cin, **kw):
    return check(M=B * h * w, N=64, K=9 * cin, a_mode=G.OPA_IM2COL, conv=(B, h, w, cin, G.NONE), lda=cin,
                 ldb=9 * cin, ldc=64, agn_gamma=A16, agn_beta=A16, agn_eps=1e-5, **kw)


def test_agn_table_capacity_is_validated():
    """Finding 1: the per-(image, channel) coefficient table of the images a tile reads must fit the LDS
    behind the ring (32 KiB + nimg cin 8 bytes <= 156 KiB).  The launch used to refuse it after the
    validation had answered "valid"; now encdiff_gemm_check refuses it (ERR_SHAPE), hence encdiff_gemm
    before it launches anything."""
    fits = lambda B, h, w, cin: 32768 + min(63 // (h * w) + 2, B) * cin * 8 <= 156 * 1024
    for B, h, w, cin in ((16, 2, 2, 960), (17, 2, 2, 928), (17, 2, 2, 960), (32, 2, 2, 1024), (64, 1, 1, 256),
                         (65, 1, 1, 224), (65, 1, 1, 256), (70, 1, 1, 512), (4, 4, 4, 1024), (70, 1, 1, 64)):
        rc = agn_check(B, h, w, cin)
        assert (rc == 0) == fits(B, h, w, cin), (B, h, w, cin, rc)
        if rc:
            assert rc == S.ERR_SHAPE


def test_vector_only_pointers_must_be_aligned():
    """Finding 2: aux (GEGLU's y output / f input), C under the GEGLU modes and ln_y are read and written
    in 16-byte vectors on every path (there is no scalar form), so the contract requires them 16-byte
    aligned: a misaligned pointer is ERR_ARG, on the host."""
    gg = dict(M=64, N=128, K=64, lda=64, ldb=64, ldc=128, c_mode=FR.OUT_BF16_GEGLU, ld_aux=64)
    assert check(aux=A16, **gg) == 0
    assert check(aux=A16 + 2, **gg) == S.ERR_ARG
    assert check(aux=A16 + 8, **gg) == S.ERR_ARG
    assert check(aux=A16, **{**gg, "c": A16 + 8}) == S.ERR_ARG
    gb = dict(M=64, N=64, K=64, lda=64, ldb=64, ldc=128, b_mode=G.OPB_ROWN, c_mode=FR.OUT_BF16_GEGLU_BWD, ld_aux=128)
    assert check(aux=A16, **gb) == 0
    assert check(aux=A16 + 4, **gb) == S.ERR_ARG
    ln = dict(M=64, N=64, K=64, lda=64, ldb=64, ldc=64, ln_gamma=A16, ln_beta=A16, ln_stats=A16, ld_ln_y=64,
              ln_eps=1e-5)
    assert check(ln_y=A16, **ln) == 0
    assert check(ln_y=A16 + 2, **ln) == S.ERR_ARG
    assert check(ln_y=A16 + 8, **ln) == S.ERR_ARG


def test_lna_serves_bf16_output_only():
    """Finding 3: the header said 'bf16 / GEGLU output'; the validation admits OUT_BF16 only (the GEGLU
    epilogue was never reached with the LayerNorm staging).  The header now says what the check does."""
    ln = dict(M=64, N=128, K=64, lda=64, ldb=64, ldc=128, lna_gamma=A16, lna_beta=A16, lna_eps=1e-5)
    assert check(**ln) == 0
    assert check(c_mode=FR.OUT_BF16_GEGLU, aux=A16, ld_aux=64, **ln) == S.ERR_ARG
    assert check(c_mode=G.OUT_F32, **ln) == S.ERR_ARG
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "encdiff_hip.h")).read()
    assert "OPA_ROWK x OPB_ROWK (OUT_BF16 only" in hdr and "bf16 / GEGLU output" not in hdr


# ====================================================================== 3. the bounds are sharp
def _sharp(kind, names, muts, run):
    """run(name, mutate) -> (fraction outside the bound, fraction of the bound the result uses)"""
    worst = {m: 0.0 for m in muts}
    for name in names:
        frac, used = run(name, None)
        print(f"{kind} {name}: model outside {frac:.3f}, uses {used:.2f} of the bound")
        assert frac == 0.0, f"{kind} {name}: the kernel model leaves the bound ({used:.2f} of it)"
        for m in muts:
            f, _ = run(name, m)
            if f is not None:
                print(f"{kind} {name}: mutation {m} outside the bound on {f:.3f} of the elements")
                worst[m] = max(worst[m], f)
    for m, f in worst.items():
        assert f >= 0.5, f"{kind}: mutation {m} exceeds the bound on only {f:.3f} of the elements of its best case"


def test_agn_bound_is_sharp():
    cache = {}

    def run(name, mutate):
        if name not in cache:
            I = FR.agn_inputs(name, strided)
            cache[name] = (I, FR.agn_bound(I))
            b = cache[name][1]
            share = (b.st / b.rnd.clamp_min(1e-300)).max().item()
            print(f"AGN {name}: |mean| / std <= {b.cond:.1f}, statistics slack / rounding term <= {share:.4f}")
            assert b.cond > 4 or share <= 1 / 8
        I, b = cache[name]
        if mutate in ("film_swap", "no_one_plus") and I.film is None or mutate == "no_silu" and not I.silu:
            return None, None
        out = FR.agn_model(I, mutate).double()
        return FR.exceeds(out, b.ref, b.tol), ((out - b.ref).abs() / b.tol).max().item()
    _sharp("AGN", FR.AGN_MUT_CASES, FR.AGN_MUTATIONS, run)


@pytest.mark.parametrize("name", [n for n in FR.AGN_CASES if n not in FR.AGN_MUT_CASES])
def test_agn_model_inside_bound(name):
    I = FR.agn_inputs(name, strided)
    b = FR.agn_bound(I)
    assert FR.exceeds(FR.agn_model(I), b.ref, b.tol) == 0.0
    share = (b.st / b.rnd.clamp_min(1e-300)).max().item()
    print(f"AGN {name}: |mean| / std <= {b.cond:.1f}, statistics slack / rounding term <= {share:.4f}")
    if b.cond <= 4:
        assert share <= 1 / 8


def test_lna_bound_is_sharp():
    cache = {}

    def run(name, mutate):
        if name not in cache:
            I = FR.lna_inputs(name, strided)
            cache[name] = (I, FR.lna_bound(I))
            b = cache[name][1]
            share = (b.st / b.rnd.clamp_min(1e-300)).max().item()
            print(f"LNA {name}: |mean| / std <= {b.cond:.1f}, statistics slack / rounding term <= {share:.4f}")
            assert b.cond > 4 or share <= 1 / 8
        I, b = cache[name]
        if mutate == "tail" and I.K % 64 == 0 or mutate == "neighbour" and I.M == 1:
            return None, None
        out = FR.lna_model(I, mutate).double()
        return FR.exceeds(out, b.ref, b.tol), ((out - b.ref).abs() / b.tol).max().item()
    _sharp("LNA", FR.LNA_MUT_CASES, FR.LNA_MUTATIONS, run)


@pytest.mark.parametrize("name", [n for n in FR.LNA_CASES if n not in FR.LNA_MUT_CASES])
def test_lna_model_inside_bound(name):
    I = FR.lna_inputs(name, strided)
    b = FR.lna_bound(I)
    assert FR.exceeds(FR.lna_model(I), b.ref, b.tol) == 0.0
    share = (b.st / b.rnd.clamp_min(1e-300)).max().item()
    print(f"LNA {name}: |mean| / std <= {b.cond:.1f}, statistics slack / rounding term <= {share:.4f}")
    if b.cond <= 4:
        assert share <= 1 / 8


def test_ln_y_bound_is_sharp():
    def run(name, mutate):
        I = FR.lny_inputs(name, strided)
        bn = G.RING_TILES[I.tile][1]
        if mutate == "div_bn" and bn == I.N or mutate == "neighbour" and I.M == 1:
            return None, None
        c = FR.linear_out(I.P, F32).to(BF16)          # a stored C; the stage is local to it
        y64, _ = FR.ln_y_stage(c, I.gamma, I.beta, I.eps, F64)
        y32, _ = FR.ln_y_stage(c, I.gamma, I.beta, I.eps, F32)
        tol, _ = FR.stored_bound(y64, y32)
        out = FR.lny_model(I, c, mutate, bn)[0].double()
        return FR.exceeds(out, y64, tol), ((out - y64).abs() / tol.clamp_min(1e-300)).max().item()
    _sharp("ln_y", FR.LNY_MUT_CASES, FR.LNY_MUTATIONS, run)


def test_geglu_bound_is_sharp():
    def run(name, mutate):
        I = FR.geglu_inputs(name, strided)
        if mutate == "gate_bias" and I.bias is None:
            return None, None
        bn = G.RING_TILES[I.tile][1]
        if mutate == "next_tile" and I.N // bn < 2:
            return None, None
        f, y = FR.geglu_model(I, mutate, bn)
        if mutate == "gate_bias":                      # a mistake of the f stage
            tol, _ = FR.stored_bound(FR.linear_out(I.P, F64), FR.linear_out(I.P, F32))
            i = I.N // 2                               # the gate half is the half it can move
            r = FR.linear_out(I.P, F64)
            return FR.exceeds(f.double()[:, i:], r[:, i:], tol[:, i:]), 0.0
        y64, y32 = FR.geglu_y(f, F64), FR.geglu_y(f, F32)
        tol, _ = FR.stored_bound(y64, y32)
        if mutate is None:
            f0 = FR.geglu_model(I)[0]
            tf, _ = FR.stored_bound(FR.linear_out(I.P, F64), FR.linear_out(I.P, F32))
            assert FR.exceeds(f0.double(), FR.linear_out(I.P, F64), tf) == 0.0
        return FR.exceeds(y.double(), y64, tol), ((y.double() - y64).abs() / tol.clamp_min(1e-300)).max().item()
    _sharp("GEGLU", FR.GEGLU_MUT_CASES, FR.GEGLU_MUTATIONS, run)


def test_geglu_bwd_bound_is_sharp():
    cache = {}

    def run(name, mutate):
        if name not in cache:
            I = FR.geglu_bwd_inputs(name, strided)
            cache[name] = (I, FR.geglu_bwd_bound(I.P, I.f, I.exact))
        I, b = cache[name]
        out = FR.geglu_bwd_model(I, mutate).double()
        i = I.N
        sl = slice(i, None) if mutate in ("no_a", "no_pdf") else slice(None)   # the half the mistake can move
        return (FR.exceeds(out[:, sl], b.ref[:, sl], b.tol[:, sl]),
                ((out - b.ref).abs() / b.tol.clamp_min(1e-300)).max().item())
    _sharp("GEGLU_BWD", FR.GEGLU_BWD_MUT_CASES, FR.GEGLU_BWD_MUTATIONS, run)


@pytest.mark.parametrize("name", [n for n, c in FR.GEGLU_BWD_CASES.items() if c["exact"]])
def test_geglu_bwd_exact_cases_carry_nothing(name):
    """Operands in {-1, 0, 1}, K <= 256: d is an integer of magnitude <= 256, which bf16 holds exactly"""
    I = FR.geglu_bwd_inputs(name, strided)
    assert I.K <= 256 and G.exact_bound(I.P) <= 256
    d = FR.linear_out(I.P, F64)
    assert torch.equal(d.to(BF16).double(), d)
    b = FR.geglu_bwd_bound(I.P, I.f, True)
    assert FR.exceeds(FR.geglu_bwd_model(I), b.ref, b.tol) == 0.0


@pytest.mark.parametrize("table,make", [(FR.LNY_CASES, FR.lny_inputs), (FR.GEGLU_CASES, FR.geglu_inputs)])
def test_exact_cases_are_exact(table, make):
    for name, c in table.items():
        if c["exact"]:
            assert G.exact_bound(make(name, strided).P) < 2 ** 24, name
