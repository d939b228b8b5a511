"""Per-element tests of the GEMM's fused norm and GEGLU stagings and epilogues on the MI355X
(csrc/gemm_tile.h): AGN (EncdiffGemmArgs.agn_*, gemm_kernel<64,64,A_IM2COL_GN,...>), LNA (lna_*,
A_ROWK_LN), ln_y (the LayerNorm epilogue of every ring tile), OUT_BF16_GEGLU and OUT_BF16_GEGLU_BWD,
against tests/gemm_fused_restate.py (written from include/encdiff_hip.h and the modules the features
replace; checked on the CPU against torch by tests/test_gemm_fused_restate.py, which also proves on
these cases' own inputs that the bounds reject a list of plausible index mistakes).

Method (the house method of test_gpu_st.py): inputs are seeded on the host (the case tables of the
restatement); every operand is placed once contiguous and once as a strided, offset view whose
surrounding elements are NaN; every output is a view inside a sentinel- or NaN-filled Guard with a padded
leading dimension, everything outside it must be unchanged; input buffers must be unchanged; each launch
runs twice and must agree bitwise; each case pins tile= and split_k=, asserts them on the built GemmArgs
and asserts the branch it names.  No tolerance is a constant: a stored bf16 value gets half a bf16 ulp of
the fp64 reference (S.bf16_store_tol), ln_stats the fp32 rule, the operand the kernel rounds without
storing (the normalised A chunk of AGN / LNA, the d of GEGLU_BWD) stays unrounded in the reference and
its half-ulp is carried through the contraction with absolute values, the statistics slack
(gemm_fused_restate.agn_stat_slack / lna_stat_slack) is carried the same way, and the floor is measured
(4 x |fp32 evaluation - fp64|).  Stage-local: ln_y / ln_stats are compared with the LayerNorm of the C
the kernel itself stored, GEGLU's y with the GEGLU of the stored f.  Exact cases (integer operands,
gemm_restate.exact_bound < 2^24): C under ln_y and f under GEGLU equal the one bf16 rounding of the fp64
result bit for bit; GEGLU_BWD with operands in {-1, 0, 1}, K <= 256 carries nothing.

Kernel branch -> test
  AGN: 16 / 4 / 1 images per tile, tiles straddling images (6x6, 3x5), B = 1, cpg 1 / 2 / 3 / 16 / 32,
    tap-uniform k-tiles or not, K tail, idle pixel lanes (cin 96), lpi clamped + several j0 passes
    (cin 512 at 2x2, cin 1024 at 4x4), 1x1 (centre tap, 64 images per tile: gst fills the ring
    scratch; ragged last tile), UP2, FiLM on / off, SiLU on / off, eps 1e-5 / 1e-6, bias, resid,
    ragged second column tile (cout 72), ld_src > cin, ld_agn_film > 2 cin ................ test_agn[...]
  AGN gn_stats slots on the stored output ............................................... test_agn[b2-16x16-c64] [b1-8x8-c64]
  AGN split_k 2: finalize pass / in-kernel fold, tickets zero ........................... test_agn[...-split2] [...-fold2]
  AGN constant image (variance 0, the clamp), |mean| / std = 16 ......................... test_agn[...-const] [...-ms16]
  AGN tile 0 -> 4, through ops.conv3x3_fwd(agn=) ......................................... test_agn_tile0_and_wrapper
  AGN refusals, the coefficient-table capacity among them (finding 1) .................... test_agn_refusals
  LNA: K 8 (lanes without a vector), K 72 (both tails), 256, 520, 1024 (the LDS maximum); M 1, 65, 100;
    N 8, 64, 72, 136; lda > K; bias, resid; a constant row; |mean| / std = 16 ............. test_lna[...]
  LNA tile 0 -> 4, through ops.linear_fwd(ln_in=) ........................................ test_lna_tile0_and_wrapper
  LNA refusals (finding 3: OUT_BF16 only) ................................................ test_lna_refusals
  ln_y: every ring tile 1-10 (TPR 2 / 4, BN 64 / 128), N 8 / 24 / 64 / 128, N 64 on a 128-wide tile,
    M 1 / 65 / 130, K 8 / 72 / 200, alpha 0.5, bias, resid, ld_ln_y > N, ln_stats rows < M only;
    the vector epilogue and each way onto the scalar one (ldc % 8, bias misaligned, resid
    misaligned, ld_resid % 8); exact cases ................................................. test_ln_y[...]
  ln_y through ops.linear_fwd_ln ......................................................... test_ln_y_wrapper
  ln_y refusals (finding 2: ln_y aligned) ................................................ test_ln_y_refusals
  OUT_BF16_GEGLU: tiles 1-10, N 128 (one column tile holds both halves) / 256 / 384, M 1 / 65 / 130,
    K 8 / 72 / 200, bias on / off, alpha 0.5, ldc > N, ld_aux > N / 2; exact cases ......... test_geglu_fwd[...]
  fused == unfused (GEGLU_FUSED off) bitwise, through ops.linear_fwd_geglu ................ test_geglu_fwd[...] (alpha 1)
  GEGLU forward refusals (finding 2: aux and c aligned) ................................... test_geglu_fwd_refusals
  OUT_BF16_GEGLU_BWD alone: tiles 1-10, inner N 8 / 72 / 128 / 200 (ragged column tiles, the col >= N
    guard), M 1 / 65 / 130, K 8 / 72 / 256, ld_aux > 2 N, ldc > 2 N, gates 0, -0, +-6, +-30;
    exact cases ........................................................................... test_geglu_bwd[...]
  as the input-gradient half of gemm_pair (ops.linear_bwd_geglu), both halves bitwise two separate
    launches, fused == unfused bitwise .................................................... test_geglu_bwd[...-pair]
  GEGLU backward refusals ................................................................. test_geglu_bwd_refusals

Three findings made while reading the kernels for these tests, each settled: (1) the AGN coefficient-table capacity is now part of the launch
validation (gemm_plan.h agn_lds_bytes, shared with launch_agn): encdiff_gemm_check and encdiff_gemm refuse
the same problems, nothing is launched (test_agn_refusals; the host arithmetic in
test_gemm_fused_restate.py).  (2) aux, C under the GEGLU modes and ln_y have no scalar path -- every access
is a 16-byte vector -- so the contract requires them 16-byte aligned and a misaligned pointer is
ENCDIFF_ERR_ARG (the *_refusals tests; never launched).  (3) LNA serves OUT_BF16 only; the header said
"bf16 / GEGLU output" and now says what the validation does (test_lna_refusals).

Measured on the MI355X: 164 cases, 1.2 s of test time for the file (3.1 s with the library load and the
collection); the slowest case 0.47 s (the first, which loads the library), every other below 0.1 s.
Per feature and output -- largest floor (4 x |torch fp32 - fp64|) / largest |out - ref| / largest fraction
of the bound used.  A stored bf16 stage with nothing carried uses all of its bound by construction (some
element always rounds at half an ulp); the stages that carry an unstored rounding stay inside it.
  AGN    c 1.3e-05 / 1.8e-02 / 0.49        gn_stats slots 5.2e-05 / 1.3e-05 / 0.17
  LNA    c 1.1e-05 / 1.6e-02 / 0.86 (K = 8; every other case below 0.50)
  ln_y   C 6.5e-06 / 3.1e-02 / 1.00        ln_y 2.9e-06 / 1.6e-02 / 1.00     ln_stats 9.2e-07 / 2.2e-07 (fp32 rule)
  GEGLU  f 6.1e-06 / 1.6e-02 / 1.00        y 1.1e-04 / 2.8e+01 / 1.00 (the exact cases' f reaches the hundreds)
  GEGLU_BWD  df 4.1e-05 / 4.4e-01 / 1.00   pair: dw 1.7e-05 / 3.0e-06, db 3.6e-06 / 8.9e-07 (fp32 rule)
Norm cases (dense and strided placements agree): largest |mean| / std of the case's groups or rows, the
statistics slack as a share of the carried rounding term (capped at 1/8 where |mean| / std <= 4), the
fraction of the bound the kernel used.
  agn b6-4x4-c64 3.0 0.013 0.39        b3-2x2-c32 18.9 0.193 0.44       b2-8x8-c96 2.2 0.009 0.40
      b20-1x1-c64 1729 9.46 0.39       b2-6x6-c64 2.1 0.011 0.35        b2-16x16-c64 2.0 0.014 0.42
      b70-1x1-c64 2144 65.6 0.45       b16-2x2-c512 2.4 0.007 0.21      b4-4x4-c1024 2.1 0.013 0.11
      b5-3x5-c32 3.0 0.012 0.40        b1-8x8-c64 1.7 0.010 0.49        b3-6x6-c32 2.4 0.026 0.43
      b8-up4x4-c64 7.1 0.035 0.32      b2-up16x16-c32 2.2 0.026 0.40    b4-8x8-c128-split2 2.0 0.007 0.33
      b4-8x8-c128-fold2 2.1 0.008 0.37 b4-4x4-c64-const 237 1.24 0.33   b4-4x4-c64-ms16 24.0 0.85 0.29
  lna m100-k8-n72 3.1 0.005 0.86       m70-k72-n64 1.2 0.003 0.50       m65-k256-n136 1.1 0.006 0.32
      m1-k1024-n64 0.6 0.014 0.08      m64-k520-n8 1.1 0.012 0.21       m65-k72-n64-const 474 1.48 0.48
      m65-k256-n64-ms16 17.6 0.71 0.21
(The 1x1 and 2x2 cases have 2 to 8 values per group, so a group's sample |mean| / std is large whatever the
inputs' nominal one; they, the constant image / row and the ms16 cases are exempt from the cap and still
inside the derived bound.)  The paired GEGLU backward runs as one gemm2_kernel grid (weight gradient on
tile 4, split 1).
No kernel bug was found while writing these tests; what they found is host side, the three findings above.
"""
import ctypes
import time

import pytest
import torch

import elementwise_restate as R
import gemm_fused_restate as FR
import gemm_restate as G
import st_restate as S
import test_gpu_st as T
from test_gpu_elementwise import BF16, F32, F64, SENT, Guard, _gen, assert_f32_rule, dev, place, rnd  # noqa: F401
from test_gpu_st import Inputs, bound, carried, nan_guard, twice  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHARE = {}   # norm case -> (|mean| / std, statistics slack / rounding term, fraction of the bound used)
TIMES = {}


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    L = ops.L
    assert (L.OUT_BF16_GEGLU, L.OUT_BF16_GEGLU_BWD) == (FR.OUT_BF16_GEGLU, FR.OUT_BF16_GEGLU_BWD)
    assert ops.GEGLU_FUSED and ops.LN_FUSED and ops.PAIR
    ops.ensure_scratch()
    t0 = time.time()
    yield ops
    ops.flush()
    torch.cuda.synchronize()
    ops._workspace().zero_()
    print(f"\nfile wall time {time.time() - t0:.1f} s; slowest cases: "
          + ", ".join(f"{k} {v:.2f} s" for k, v in sorted(TIMES.items(), key=lambda kv: -kv[1])[:3]))
    print("stage: largest floor / largest |out - ref| / largest fraction of the bound used")
    for k in sorted(T.STATS):
        if k.split(".")[0] in ("agn", "lna", "lny", "geglu", "gbwd"):
            print(f"  {k:10s} {T.STATS[k][0]:.2e} {T.STATS[k][1]:.2e} {T.STATS[k][2]:.3f}")
    print("norm case: |mean| / std, statistics slack / carried rounding term, fraction of the bound used")
    for k in sorted(SHARE):
        print(f"  {k:28s} {SHARE[k][0]:8.1f} {SHARE[k][1]:.4f} {SHARE[k][2]:.3f}")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    TIMES[request.node.name] = time.time() - t0


# ====================================================================== plumbing
class Placer:
    """put(kind, host tensor) of the restatement's input builders: 2-D operands contiguous or as strided,
    offset views (offset 8, stride + 24) whose surrounding elements are NaN; fp32 vectors 16 bytes into a
    NaN-filled buffer (`misalign`: the kinds placed 4 / 8 bytes off instead).  Every buffer is kept:
    unchanged() proves no launch wrote an input."""

    def __init__(self, strided, way="vec"):
        self.strided, self.way, self.inp = strided, way, Inputs()

    def mat(self, t, ld=None, left=None):
        g = Guard(t.shape[0], t.shape[1], t.dtype, strided=self.strided and ld is None, init=t.to(dev), ld=ld,
                  left=left, fill=NAN)
        self.inp.keep(g.buf)
        return g.view

    def vec(self, t, left=4):
        g = Guard(1, t.numel(), F32, init=t.reshape(1, -1).to(dev), left=left, ld=left + t.numel(), fill=NAN)
        self.inp.keep(g.buf)
        return g.view[0]

    def __call__(self, kind, t):
        if kind == "film":           # [B][2 cin + 8]: the builder's own NaN columns make ld_agn_film > 2 cin
            return self.inp.keep(t.to(dev))
        if kind == "vec":
            return self.vec(t)
        if kind == "bias":
            return self.vec(t, left=1 if self.way == "bias_misaligned" else 4)
        if kind == "resid_way":
            n = t.shape[1]
            if self.way == "resid_misaligned":
                return self.mat(t, n + 8, 4)
            if self.way == "ld_resid":
                return self.mat(t, n + 4, 0)
        return self.mat(t)


def ptr(t):
    return None if t is None else t.data_ptr()


def tickets_zero(O):
    return int(O._counters().abs().sum()) == 0


def launch(O, args, what):
    """encdiff_gemm on built GemmArgs: slabs NaN beforehand, tickets zero before and after"""
    O.flush()
    nws = O.ws_floats(args)
    if nws:
        O._workspace()[:nws].fill_(NAN)
    assert tickets_zero(O)
    O.check(O.lib.encdiff_gemm(ctypes.byref(args), O._s()), "encdiff_gemm")
    torch.cuda.synchronize()
    assert tickets_zero(O), f"{what}: tickets not left zero"


def pinned(args, tile, split, what, fold=False):
    assert (args.tile, args.split_k) == (tile, split), f"{what}: plan changed to {(args.tile, args.split_k)}"
    assert bool(args.split_counters) == bool(fold), f"{what}: tickets {bool(args.split_counters)}, case needs {fold}"


def refuse(O, args, guards, what, rc=None):
    """The validation (host only) must refuse first; only then is encdiff_gemm called, which must refuse
    the same way (HipError) and leave every output as it was."""
    got = O.lib.encdiff_gemm_check(ctypes.byref(args), None)
    assert got != 0, f"{what}: encdiff_gemm_check admits it"
    if rc is not None:
        assert got == rc, f"{what}: refused with {got}, expected {rc}"
    ran = O.lib.encdiff_gemm(ctypes.byref(args), O._s())
    assert ran == got, f"{what}: encdiff_gemm answers {ran}, encdiff_gemm_check {got}"
    with pytest.raises(O.L.HipError):
        O.check(ran, what)
    torch.cuda.synchronize()
    for g in guards:
        assert R.same_bits(g.buf, g.before), f"{what}: a refused launch wrote an output"


def exact_same(what, out, ref64):
    want = ref64.to(F32).to(BF16)
    bad = ((out + 0) != (want + 0)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ from the one rounding of the exact result, " \
                             f"first {bad[0].tolist()}: {out[tuple(bad[0])].item()} vs {want[tuple(bad[0])].item()}"


def share(name, b, out):
    sh = (b.st / b.rnd.clamp_min(1e-300)).max().item()
    used = ((out.double() - b.ref).abs() / b.tol).max().item()
    SHARE[name] = (b.cond, sh, used)
    print(f"{name}: |mean| / std <= {b.cond:.1f}, statistics slack / rounding term <= {sh:.4f}, bound used {used:.3f}")
    if b.cond <= 4:
        assert sh <= 1 / 8, f"{name}: the statistics slack is {sh:.3f} of the rounding term"


# ====================================================================== AGN
def agn_args(O, I, c, gn=None, split=1, fold=False, lib_tile=4):
    cs = I.case
    cg = O.L.ConvGeom(batch=I.B, h=I.hh, w=I.ww, cin=I.cin, resample=I.resample, ld_src=I.x.stride(0))
    args = O.gemm_args(I.M, I.cout, I.K, I.x, I.x.stride(0), I.w, I.w.stride(0), c, c.stride(0),
                       a_mode=G.OPA_IM2COL, conv=cg, bias=I.bias, resid=I.resid,
                       ld_resid=I.resid.stride(0) if I.resid is not None else 0, tile=4, split_k=split,
                       gn_stats=gn, agn=(I.gamma, I.beta, I.film, I.eps, I.silu), fold=fold)
    pinned(args, 4, split, I.name, fold)
    assert args.ld_agn_film == (2 * I.cin + 8 if cs["film"] else 0) and args.conv.ld_src == I.x.stride(0)
    args.tile = lib_tile
    return args


def agn_branch(I):
    """What the case claims to reach, from the header's description of the geometry"""
    np_ = 256 // (I.cin // 8)
    lpi = max(np_ // I.nimg, 1)
    return dict(nimg=I.nimg, lpi=lpi, passes=-(-I.nimg // (np_ // lpi)),
                idle=256 - np_ * (I.cin // 8), tapk=G.tap_uniform(I.cin), ktail=I.K % 64 != 0,
                ragged_m=I.M % 64 != 0, ragged_n=I.cout % 64 != 0)


AGN_EXPECT = {
    "b6-4x4-c64": dict(nimg=4, tapk=True, ktail=False), "b3-2x2-c32": dict(tapk=False, ktail=True, ragged_m=True),
    "b2-8x8-c96": dict(idle=4, tapk=False, ragged_n=True, nimg=1), "b20-1x1-c64": dict(nimg=20, ragged_m=True),
    "b2-6x6-c64": dict(nimg=2, ragged_m=True), "b2-16x16-c64": dict(nimg=1, lpi=32),
    "b70-1x1-c64": dict(nimg=64, lpi=1, passes=2, ragged_m=True), "b16-2x2-c512": dict(nimg=16, lpi=1, passes=4),
    "b4-4x4-c1024": dict(nimg=4, lpi=1, passes=2), "b5-3x5-c32": dict(nimg=5, ragged_m=True, ragged_n=True),
    "b1-8x8-c64": dict(nimg=1), "b8-up4x4-c64": dict(nimg=4), "b2-up16x16-c32": dict(nimg=1),
}


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("name", list(FR.AGN_CASES))
def test_agn(O, name, strided):
    """Catches: a coefficient row of the neighbouring image, a group index off by one, FiLM scale / shift
    exchanged or without the 1 +, SiLU dropped, unbiased variance (test_gemm_fused_restate.py shows each
    leaves this bound on most elements), the j0 loop dropping a pass (an image's coefficients never
    written), a padding tap transformed (it must stay zero), statistics over the wrong pixel count under
    UP2, a slot of gn_stats from the unrounded value."""
    pl = Placer(strided)
    I = FR.agn_inputs(name, pl)
    cs = I.case
    br = agn_branch(I)
    for k, v in AGN_EXPECT.get(name, {}).items():
        assert br[k] == v, f"{name}: branch changed: {k} = {br[k]}, this case needs {v}"

    def run():
        o = {"c": Guard(I.M, I.cout, BF16, strided=True, init=torch.full((I.M, I.cout), NAN, device=dev))}
        if cs["gn"]:
            o["gn"] = Guard(2 * (I.M // 64), I.cout, F32, strided=True,
                            init=torch.full((2 * (I.M // 64), I.cout), NAN, device=dev))
        args = agn_args(O, I, o["c"].view, o["gn"].view if cs["gn"] else None, cs["split"], cs["fold"])
        launch(O, args, name)
        for g in o.values():
            g.check()
        return o
    o, _ = twice(run)
    pl.inp.unchanged()
    b = FR.agn_bound(I)
    share(f"agn {name}" + ("-s" if strided else ""), b, o.c)
    bound(f"agn {name} agn.c", o.c, (b.ref, b.ref32), slack=b.rnd + b.st)
    if cs["gn"]:
        bound(f"agn {name} agn.gn", o.gn, lambda d: S.gn_sums(o.c, d), store=False)


def test_agn_tile0_and_wrapper(O):
    """tile 0 is planned onto tile 4 by the library (bitwise the pinned launch); ops.conv3x3_fwd(agn=)
    reaches the same kernel under its own split plan (inside the same bound)."""
    name = "b6-4x4-c64"
    pl = Placer(True)
    I = FR.agn_inputs(name, pl)
    outs = []
    for lib_tile in (4, 0):
        c = Guard(I.M, I.cout, BF16, strided=True, init=torch.full((I.M, I.cout), NAN, device=dev))
        launch(O, agn_args(O, I, c.view, lib_tile=lib_tile), name)
        c.check()
        outs.append(c)
    assert R.same_bits(outs[0].buf, outs[1].buf)
    c = Guard(I.M, I.cout, BF16, strided=True, init=torch.full((I.M, I.cout), NAN, device=dev))
    O.conv3x3_fwd(I.x, O.Geom(I.B, I.hh, I.ww), I.cin, I.w, c.view, bias=I.bias,
                  agn=(I.gamma, I.beta, I.film, I.eps, I.silu))
    torch.cuda.synchronize()
    c.check()
    pl.inp.unchanged()
    b = FR.agn_bound(I)
    assert FR.exceeds(c.view, b.ref, b.tol) == 0.0


def test_agn_refusals(O):
    """Refused by the validation, on the host, with the outputs untouched."""
    L = O.L
    pl = Placer(False)
    I = FR.agn_inputs("b6-4x4-c64", pl)
    c = Guard(I.M, I.cout, BF16, init=torch.zeros(I.M, I.cout, dtype=BF16, device=dev))
    st = nan_guard(I.M, 2)

    def base():
        return agn_args(O, I, c.view)

    def mut(what, rc=None, **kw):
        a = base()
        for k, v in kw.items():
            if k.startswith("conv_"):
                setattr(a.conv, k[5:], v)
            else:
                setattr(a, k, v)
        refuse(O, a, [c, st], "agn " + what, rc)

    assert O.lib.encdiff_gemm_check(ctypes.byref(base()), None) == 0
    mut("DOWN2", conv_resample=L.RESAMPLE_DOWN2)
    mut("STRIDE2", S.ERR_UNSUPPORTED, conv_resample=L.RESAMPLE_STRIDE2)
    mut("cin 48", S.ERR_SHAPE, conv_cin=48, K=9 * 48)
    mut("cin 1056", S.ERR_SHAPE, conv_cin=1056, K=9 * 1056)
    mut("tile 3", S.ERR_UNSUPPORTED, tile=3)
    mut("c_mode F32", S.ERR_ARG, c_mode=G.OUT_F32)
    mut("with ln_y", S.ERR_ARG, ln_y=ptr(c.view), ld_ln_y=64, ln_gamma=ptr(I.gamma), ln_beta=ptr(I.beta),
        ln_stats=ptr(st.view), ln_eps=1e-5)
    mut("K != 9 cin", S.ERR_SHAPE, K=9 * I.cin - 8)
    mut("M != batch h w", S.ERR_SHAPE, conv_batch=I.B + 1)
    # finding 1: the coefficient table of the images a tile reads must fit the LDS behind the ring.  The
    # validation refuses what launch_agn used to refuse after the plan had been called valid.
    for B, h, cin, fit in ((17, 2, 960, 16), (65, 1, 256, 60)):
        M = B * h * h
        x = torch.zeros(M, cin, dtype=BF16, device=dev)
        w = torch.zeros(64, 9 * cin, dtype=BF16, device=dev)
        gb = torch.ones(cin, device=dev)
        cc = Guard(M, 64, BF16, init=torch.zeros(M, 64, dtype=BF16, device=dev))
        cg = L.ConvGeom(batch=B, h=h, w=h, cin=cin, resample=0, ld_src=cin)
        a = O.gemm_args(M, 64, 9 * cin, x, cin, w, 9 * cin, cc.view, 64, a_mode=G.OPA_IM2COL, conv=cg, tile=4,
                        split_k=1, agn=(gb, gb, None, 1e-5, True))
        refuse(O, a, [cc], f"agn capacity B={B} {h}x{h} cin={cin}", S.ERR_SHAPE)
        a.conv.batch, a.M = fit, fit * h * h           # a smaller batch fits
        assert O.lib.encdiff_gemm_check(ctypes.byref(a), None) == 0


# ====================================================================== LNA
def lna_args(O, I, c, lib_tile=4):
    args = O.gemm_args(I.M, I.N, I.K, I.x, I.x.stride(0), I.w, I.w.stride(0), c, c.stride(0), bias=I.bias,
                       resid=I.resid, ld_resid=I.resid.stride(0) if I.resid is not None else 0, tile=4, split_k=1,
                       lna=(I.gamma, I.beta, I.eps))
    pinned(args, 4, 1, I.name)
    args.tile = lib_tile
    return args


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("name", list(FR.LNA_CASES))
def test_lna(O, name, strided):
    """Catches: the statistics of the neighbouring row, gamma / beta shifted by a vector, unbiased variance
    (K = 8), the K tail or a masked row normalised (a NaN or a non-zero product), lanes without a vector
    adding garbage (K = 8), a row beyond M written."""
    pl = Placer(strided)
    I = FR.lna_inputs(name, pl)
    assert (I.K % 64 != 0, I.M % 64 != 0, I.N % 64 != 0) == \
        {"m100-k8-n72": (True, True, True), "m70-k72-n64": (True, True, False), "m65-k256-n136": (False, True, True),
         "m1-k1024-n64": (False, True, False), "m64-k520-n8": (True, False, True),
         "m65-k72-n64-const": (True, True, False), "m65-k256-n64-ms16": (False, True, False)}[name]
    if strided:
        assert I.x.stride(0) > I.K

    def run():
        o = {"c": Guard(I.M, I.N, BF16, strided=True, init=torch.full((I.M, I.N), NAN, device=dev))}
        launch(O, lna_args(O, I, o["c"].view), name)
        o["c"].check()
        return o
    o, _ = twice(run)
    pl.inp.unchanged()
    b = FR.lna_bound(I)
    share(f"lna {name}" + ("-s" if strided else ""), b, o.c)
    bound(f"lna {name} lna.c", o.c, (b.ref, b.ref32), slack=b.rnd + b.st)


def test_lna_tile0_and_wrapper(O):
    name = "m70-k72-n64"
    pl = Placer(True)
    I = FR.lna_inputs(name, pl)
    outs = []
    for lib_tile in (4, 0):
        c = Guard(I.M, I.N, BF16, strided=True, init=torch.full((I.M, I.N), NAN, device=dev))
        launch(O, lna_args(O, I, c.view, lib_tile), name)
        c.check()
        outs.append(c)
    c = Guard(I.M, I.N, BF16, strided=True, init=torch.full((I.M, I.N), NAN, device=dev))
    O.linear_fwd(I.x, I.w, c.view, bias=I.bias, resid=I.resid, ln_in=(I.gamma, I.beta, I.eps))
    torch.cuda.synchronize()
    c.check()
    pl.inp.unchanged()
    assert R.same_bits(outs[0].buf, outs[1].buf) and R.same_bits(outs[0].buf, c.buf)


def test_lna_refusals(O):
    pl = Placer(False)
    I = FR.lna_inputs("m70-k72-n64", pl)
    c = Guard(I.M, I.N, BF16, init=torch.zeros(I.M, I.N, dtype=BF16, device=dev))
    y = Guard(I.M, I.N, BF16, init=torch.zeros(I.M, I.N, dtype=BF16, device=dev))
    st = nan_guard(I.M, 2)

    def mut(what, rc=None, **kw):
        a = lna_args(O, I, c.view)
        for k, v in kw.items():
            setattr(a, k, v)
        refuse(O, a, [c, y, st], "lna " + what, rc)

    assert O.lib.encdiff_gemm_check(ctypes.byref(lna_args(O, I, c.view)), None) == 0
    mut("K 1032", S.ERR_SHAPE, K=1032)
    mut("K 12", S.ERR_SHAPE, K=12)
    mut("lda % 8", S.ERR_SHAPE, lda=I.x.stride(0) + 4)
    mut("a misaligned", S.ERR_SHAPE, a=ptr(I.x) + 8)
    mut("tile 3", S.ERR_UNSUPPORTED, tile=3)
    mut("split 2", S.ERR_ARG, split_k=2, workspace=O._workspace().data_ptr())
    mut("c_mode F32", S.ERR_ARG, c_mode=G.OUT_F32)
    # finding 3: the header promised GEGLU output; the validation admits OUT_BF16 only, the header now agrees
    # (N = 128 without resid is what the GEGLU mode itself admits: the refusal is the LayerNorm staging's)
    mut("c_mode GEGLU", S.ERR_ARG, c_mode=FR.OUT_BF16_GEGLU, aux=ptr(y.view), ld_aux=64, N=128, ldc=128, resid=None)
    mut("with agn", S.ERR_ARG, agn_gamma=ptr(I.gamma), agn_beta=ptr(I.beta))
    mut("with ln_y", S.ERR_ARG, ln_y=ptr(y.view), ld_ln_y=I.N, ln_gamma=ptr(I.gamma), ln_beta=ptr(I.beta),
        ln_stats=ptr(st.view), ln_eps=1e-5)


# ====================================================================== ln_y
def lny_out(I):
    c = I.case
    ldc = (I.N + 4, 0) if c["way"] == "ldc" else (None, None)
    o = {"c": Guard(I.M, I.N, BF16, strided=ldc[0] is None, ld=ldc[0], left=ldc[1],
                    init=torch.full((I.M, I.N), NAN, device=dev)),
         "y": Guard(I.M, I.N, BF16, strided=True, init=torch.full((I.M, I.N), NAN, device=dev)),
         "st": nan_guard(I.M + 3, 2)}
    return o


def lny_args(O, I, o):
    args = O.gemm_args(I.M, I.N, I.K, I.x, I.x.stride(0), I.w, I.w.stride(0), o["c"].view, o["c"].view.stride(0),
                       alpha=I.alpha, bias=I.bias, resid=I.resid,
                       ld_resid=I.resid.stride(0) if I.resid is not None else 0, tile=I.tile, split_k=1,
                       ln=(I.gamma, I.beta, o["y"].view, o["st"].view[:I.M], I.eps))
    pinned(args, I.tile, 1, I.name)
    return args


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("name", list(FR.LNY_CASES))
def test_ln_y(O, name, strided):
    """Catches: the variance divided by BN instead of N, the statistics of the neighbouring row, gamma /
    beta shifted by a vector, unbiased variance, the scalar epilogue feeding the LayerNorm unrounded
    values (the exact cases: C then differs from its stored rounding), a lane of a row skipped (TPR 2 /
    4), ln_stats written for rows >= M."""
    c = FR.LNY_CASES[name]
    pl = Placer(strided, c["way"])
    I = FR.lny_inputs(name, pl)
    BM, BN, _, _ = G.tile_shape(I.tile)
    assert I.N <= BN

    def run():
        o = lny_out(I)
        args = lny_args(O, I, o)
        vec = G.epilogue_vec(I.N, args.ldc, args.c, args.bias or None, args.resid or None, args.ld_resid)
        assert vec == (c["way"] == "vec"), f"{name}: epilogue path changed"
        assert args.ld_ln_y > I.N and args.ln_y % 16 == 0
        launch(O, args, name)
        for g in o.values():
            g.check()
        return o
    o, _ = twice(run)
    pl.inp.unchanged()
    st = o.st[:I.M]
    assert torch.isnan(o.st[I.M:]).all(), "ln_stats written beyond M"
    r64, r32 = FR.linear_out(I.P, F64), FR.linear_out(I.P, F32)
    if c["exact"]:
        assert G.exact_bound(I.P) < 2 ** 24
        exact_same(f"ln_y {name} C", o.c, r64)
    else:
        bound(f"lny {name} lny.c", o.c, (r64, r32))
    f = lambda d: FR.ln_y_stage(o.c, I.gamma, I.beta, I.eps, d)
    bound(f"lny {name} lny.y", o.y, (f(F64)[0], f(F32)[0]))
    T.f32_rule(f"lny {name} lny.stats", st, lambda d: f(d)[1])


def test_ln_y_wrapper(O):
    """ops.linear_fwd_ln at a sampling batch takes tile 4 (N <= 64) / 3 (N <= 128): bitwise the pinned launch"""
    for name, tile in (("t4-m65-n64", 4), ("t3-m65-n128", 3)):
        pl = Placer(True)
        I = FR.lny_inputs(name, pl)
        assert I.tile == tile and I.alpha == 1.0
        o = lny_out(I)
        launch(O, lny_args(O, I, o), name)
        w = lny_out(I)
        O.linear_fwd_ln(I.x, I.w, w["c"].view, I.gamma, I.beta, w["y"].view, w["st"].view[:I.M], I.eps, bias=I.bias,
                        resid=I.resid)
        torch.cuda.synchronize()
        for k in o:
            w[k].check()
            assert R.same_bits(o[k].buf, w[k].buf), f"{name}: {k} differs between the wrapper and the pinned launch"
        pl.inp.unchanged()


def test_ln_y_refusals(O):
    pl = Placer(False)
    I = FR.lny_inputs("t4-m65-n64", pl)
    o = lny_out(I)

    def mut(what, rc=None, **kw):
        a = lny_args(O, I, o)
        for k, v in kw.items():
            setattr(a, k, v)
        refuse(O, a, list(o.values()), "ln_y " + what, rc)

    assert O.lib.encdiff_gemm_check(ctypes.byref(lny_args(O, I, o)), None) == 0
    mut("N > BN", S.ERR_ARG, N=72)
    mut("N % 8", S.ERR_ARG, N=60)
    mut("tile 0", S.ERR_ARG, tile=0)
    mut("split 2", S.ERR_ARG, split_k=2, workspace=O._workspace().data_ptr())
    mut("c_mode F32", S.ERR_ARG, c_mode=G.OUT_F32)
    mut("no gamma", S.ERR_ARG, ln_gamma=None)
    mut("no beta", S.ERR_ARG, ln_beta=None)
    mut("no stats", S.ERR_ARG, ln_stats=None)
    mut("ld_ln_y % 8", S.ERR_ARG, ld_ln_y=I.N + 4)
    # finding 2: ln_y is written in 16-byte vectors on both epilogue paths
    mut("ln_y misaligned by 2", S.ERR_ARG, ln_y=ptr(o["y"].view) + 2)
    mut("ln_y misaligned by 8", S.ERR_ARG, ln_y=ptr(o["y"].view) + 8)


# ====================================================================== GEGLU forward
def geglu_out(I):
    return {"f": Guard(I.M, I.N, BF16, strided=True, init=torch.full((I.M, I.N), NAN, device=dev)),
            "y": Guard(I.M, I.N // 2, BF16, strided=True, init=torch.full((I.M, I.N // 2), NAN, device=dev))}


def geglu_args(O, I, o):
    args = O.gemm_args(I.M, I.N, I.K, I.x, I.x.stride(0), I.w, I.w.stride(0), o["f"].view, o["f"].view.stride(0),
                       c_mode=FR.OUT_BF16_GEGLU, alpha=I.alpha, bias=I.bias, tile=I.tile, split_k=1,
                       aux=o["y"].view, ld_aux=o["y"].view.stride(0))
    pinned(args, I.tile, 1, I.name)
    assert args.ldc > I.N and args.ld_aux > I.N // 2
    return args


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("name", list(FR.GEGLU_CASES))
def test_geglu_fwd(O, name, strided, monkeypatch):
    """Catches: value and gate halves exchanged, the gate of another column tile (gcol with the wrong by),
    the gate's bias read at the value's column, y formed from the unrounded f (the exact cases pin f; y is
    compared with the GEGLU of the stored f under half an ulp), a column tile of one half skipped."""
    c = FR.GEGLU_CASES[name]
    pl = Placer(strided)
    I = FR.geglu_inputs(name, pl)
    BM, BN, _, _ = G.tile_shape(I.tile)
    assert I.M % BM, "every case leaves a ragged last row tile"

    def run():
        o = geglu_out(I)
        launch(O, geglu_args(O, I, o), name)
        for g in o.values():
            g.check()
        return o
    o, guards = twice(run)
    r64, r32 = FR.linear_out(I.P, F64), FR.linear_out(I.P, F32)
    if c["exact"]:
        assert G.exact_bound(I.P) < 2 ** 24
        exact_same(f"geglu {name} f", o.f, r64)
    else:
        bound(f"geglu {name} geglu.f", o.f, (r64, r32))
    bound(f"geglu {name} geglu.y", o.y, lambda d: FR.geglu_y(o.f, d))
    if I.alpha == 1.0:   # the wrapper (its own plan) fused and unfused: bitwise
        res = []
        for fused in (True, False):
            monkeypatch.setattr(O, "GEGLU_FUSED", fused)
            w = geglu_out(I)
            O.linear_fwd_geglu(I.x, I.w, w["f"].view, w["y"].view, bias=I.bias)
            torch.cuda.synchronize()
            for g in w.values():
                g.check()
            res.append(w)
        for k in ("f", "y"):
            assert R.same_bits(res[0][k].buf, res[1][k].buf), f"{name}: {k}: fused and unfused differ"
            assert R.same_bits(res[0][k].buf, guards[k].buf), f"{name}: {k}: the wrapper and the pinned tile differ"
    pl.inp.unchanged()


def test_geglu_fwd_refusals(O):
    pl = Placer(False)
    I = FR.geglu_inputs("t4-m65-n128", pl)
    o = geglu_out(I)
    r = Guard(I.M, I.N, BF16, init=torch.zeros(I.M, I.N, dtype=BF16, device=dev))

    def mut(what, rc=None, **kw):
        a = geglu_args(O, I, o)
        for k, v in kw.items():
            setattr(a, k, v)
        refuse(O, a, list(o.values()), "geglu " + what, rc)

    assert O.lib.encdiff_gemm_check(ctypes.byref(geglu_args(O, I, o)), None) == 0
    mut("N % 128", S.ERR_ARG, N=64)
    mut("resid", S.ERR_ARG, resid=ptr(r.view), ld_resid=I.N)
    mut("split 2", S.ERR_ARG, split_k=2)
    mut("aux NULL", S.ERR_ARG, aux=None)
    mut("ld_aux % 8", S.ERR_ARG, ld_aux=I.N // 2 + 4)
    mut("b_mode ROWN", S.ERR_ARG, b_mode=G.OPB_ROWN)
    mut("a_mode ROWM", None, a_mode=G.OPA_ROWM)
    # finding 2: y and f are written in 16-byte vectors only
    mut("aux misaligned by 2", S.ERR_ARG, aux=ptr(o["y"].view) + 2)
    mut("aux misaligned by 8", S.ERR_ARG, aux=ptr(o["y"].view) + 8)
    mut("c misaligned by 8", S.ERR_ARG, c=ptr(o["f"].view) + 8)


# ====================================================================== GEGLU backward
def gbwd_args(O, I, df, off=0):
    args = O.gemm_args(I.M, I.N, I.K, I.dy, I.dy.stride(0), I.w, I.w.stride(0), df, df.stride(0), b_mode=G.OPB_ROWN,
                       c_mode=FR.OUT_BF16_GEGLU_BWD, tile=I.tile, split_k=1, aux=I.f, ld_aux=I.f.stride(0),
                       ws_offset=off)
    pinned(args, I.tile, 1, I.name)
    return args


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("name", list(FR.GEGLU_BWD_CASES))
def test_geglu_bwd(O, name, strided, monkeypatch):
    """Catches: dg without the factor a, gelu' without the x pdf term, the gate read at column col instead
    of N + col (each leaves the bound on most elements: test_gemm_fused_restate.py), d not rounded to bf16
    first (the unfused pair differs bitwise), a ragged column tile writing past column N into the gate
    half, f read at the wrong leading dimension."""
    c = FR.GEGLU_BWD_CASES[name]
    pl = Placer(strided)
    I = FR.geglu_bwd_inputs(name, pl)
    if strided:
        assert I.f.stride(0) > 2 * I.N

    def run():
        o = {"df": Guard(I.M, 2 * I.N, BF16, strided=True, init=torch.full((I.M, 2 * I.N), NAN, device=dev))}
        args = gbwd_args(O, I, o["df"].view)
        assert args.ldc > 2 * I.N
        launch(O, args, name)
        o["df"].check()
        return o
    o, guards = twice(run)
    b = FR.geglu_bwd_bound(I.P, I.f, c["exact"])
    if c["exact"]:
        assert I.K <= 256 and G.exact_bound(I.P) <= 256 and float(b.rnd.max()) == 0.0
    bound(f"gbwd {name} gbwd.df", o.df, (b.ref, b.ref32), slack=b.rnd)
    if c["pair"]:
        pair_case(O, I, guards["df"], monkeypatch, name)
    pl.inp.unchanged()


def pair_case(O, I, alone, monkeypatch, name):
    """ops.linear_bwd_geglu: the GEGLU backward as the input-gradient half of a paired launch.  Both halves
    bitwise two separate launches; df bitwise the launch alone and the unfused pair."""
    g = _gen(77)
    a = rnd(g, I.M, I.N, dtype=BF16)                       # the GEGLU output the next layer read
    dw0, db0 = rnd(g, I.K, I.N), rnd(g, I.K)
    wa = O.linear_wgrad_args(I.dy, a, dw0.clone(), db0.clone())
    da = O.gemm_args(I.M, I.N, I.K, I.dy, I.dy.stride(0), I.w, I.w.stride(0), alone.view, alone.view.stride(0),
                     b_mode=G.OPB_ROWN, c_mode=FR.OUT_BF16_GEGLU_BWD, split_k=1, aux=I.f, ld_aux=I.f.stride(0))
    route = G.pair_route((wa.a_mode, wa.b_mode), wa.tile, (da.a_mode, da.b_mode), da.tile)
    print(f"{name}: weight gradient tile {wa.tile} split {wa.split_k}, input gradient tile {da.tile}, route {route}")
    assert route == "gemm2", f"{name}: the pair no longer runs as one gemm2_kernel grid ({route})"

    def both(fused, paired):
        monkeypatch.setattr(O, "GEGLU_FUSED", fused)
        monkeypatch.setattr(O, "PAIR", paired)
        df = Guard(I.M, 2 * I.N, BF16, strided=True, init=torch.full((I.M, 2 * I.N), NAN, device=dev))
        d_a = Guard(I.M, I.N, BF16, strided=True)
        dw, db = dw0.clone(), db0.clone()
        O.linear_bwd_geglu(I.dy, I.w, a, I.f, df.view, dw, db, d_a=d_a.view)
        O.flush()
        torch.cuda.synchronize()
        df.check()
        assert tickets_zero(O)
        return df, dw, db
    pf, pw, pb = both(True, True)
    sf, sw, sb = both(True, False)
    uf, uw, ub = both(False, True)
    assert R.same_bits(pf.buf, sf.buf) and R.same_bits(pw, sw) and R.same_bits(pb, sb), \
        f"{name}: the paired launch and two separate launches differ"
    assert R.same_bits(pf.buf, uf.buf) and R.same_bits(pw, uw) and R.same_bits(pb, ub), \
        f"{name}: fused and unfused differ"
    assert R.same_bits(pf.view.contiguous(), alone.view.contiguous()), f"{name}: the pair's df and the launch alone differ"
    # the weight-gradient half per element: dw += dy^T a, db += column sums of dy
    T.f32_rule(f"gbwd {name} gbwd.dw", pw, lambda d: dw0.to(d) + I.dy.to(d).t() @ a.to(d))
    T.f32_rule(f"gbwd {name} gbwd.db", pb, lambda d: db0.to(d) + I.dy.to(d).sum(0))


def test_geglu_bwd_refusals(O):
    pl = Placer(False)
    I = FR.geglu_bwd_inputs("t4-m65-n72-exact", pl)
    df = Guard(I.M, 2 * I.N, BF16, init=torch.zeros(I.M, 2 * I.N, dtype=BF16, device=dev))

    def mut(what, rc=None, **kw):
        a = gbwd_args(O, I, df.view)
        for k, v in kw.items():
            setattr(a, k, v)
        refuse(O, a, [df], "geglu_bwd " + what, rc)

    assert O.lib.encdiff_gemm_check(ctypes.byref(gbwd_args(O, I, df.view)), None) == 0
    mut("resid", S.ERR_ARG, resid=ptr(df.view), ld_resid=2 * I.N)
    mut("split 2", S.ERR_ARG, split_k=2)
    mut("aux NULL", S.ERR_ARG, aux=None)
    mut("N % 8", None, N=I.N - 4)
    mut("aux misaligned by 8", S.ERR_ARG, aux=ptr(I.f) + 8)
    mut("c misaligned by 2", S.ERR_ARG, c=ptr(df.view) + 2)
