"""Per-element tests of the fused SpatialTransformer kernels on the MI355X, through ops.st_*:
csrc/st_fused.hip (encdiff_st_tail_fwd, encdiff_st_head_fwd), csrc/st_bwd.hip (encdiff_st_tail_bwd,
encdiff_st_head_bwd) and the helpers of csrc/st_common.h, on every row tile, wave count, statistics
form and key-gradient form their entry points dispatch to.

Method: stage-local checks on the kernel's own tensors.  A chain of ten rounded stages cannot be
bounded end to end per element -- one flipped bf16 rounding early is a full ulp later -- but the
training forward writes every intermediate and the backward every gradient it computes.  So each
stage is compared with the fp64 restatement of THAT stage (tests/st_restate.py) applied to what the
kernel itself stored for the stage's inputs, under the bound of that stage's roundings
(st_restate.ST_ROUNDS, "bound helpers"): a stored bf16 value may differ by half a bf16 ulp of the
reference; an operand the kernel rounds without storing it (d_a, d_n3, d_o2, d_n2, d_n1, gn / n1 in
the forms that do not write them) is kept unrounded in the reference and its half-ulp is carried
through the consumer's contraction with absolute values; the fp32 residual stream that the next
stage reads unrounded contributes half an ulp of the saved value; fp32 outputs (s1 s2 s3 lse2, the
statistics slots, gn_stats, the LayerNorm partial rows, the dK | dV slabs) take the fp32 rule.  The
additive floor is measured, never fixed: 4 x |torch fp32 evaluation - fp64| of the same restatement.
No constant is a tolerance: the derived slacks are gelu_fast's erf error (ERF_ERR) and the fast exp's
relative error (exp_rel_of), both worked out in st_restate.py.

Every case: inputs are column views of wider buffers whose rows end in NaN columns; bf16 outputs sit
in sentinel-filled Guards with padded leading dimensions, fp32 outputs in NaN-filled Guards;
everything outside the views must be unchanged; each launch runs twice and must agree bitwise; the
case asserts its StPlan path before it launches.  An inference launch (no saves) must give `out`
(head mode: t2 / n3) bit-identical to the training launch of the same shape.

Kernel instance / branch -> test
  st_tail_kernel<64,16,4>: 1 / 4 images per tile ................ test_tail_fwd[c64-t256-B1] [c64-t16-B2] [c64-t4-B8]
  st_tail_kernel<64,64,4> + statistics (store), 1 / 4 images .... test_tail_fwd[c64-t64-B2-stats] [c64-t16-B8-stats]
  st_tail_kernel<64,64,4> by the row threshold .................. test_tail_fwd[c64-t256-B64]
  st_tail_kernel<64,32,4> add form (ST_TAIL_R32_C64 on) ......... test_tail_fwd[c64-t64-B2-r32add]
  st_tail_kernel<128,16,8> ...................................... test_tail_fwd[c128-t64-B2] [c128-t4-B4]
  st_tail_kernel<128,32,8> / <128,32,4> add form ................ test_tail_fwd[c128-t64-B2-add] [c128-t64-B128-add]
  st_tail_kernel<128,64,8> store form (ST_TAIL_STATS_ADD off) ... test_tail_fwd[c128-t64-B2-store]
  st_tail_kernel<128,64,4> ...................................... test_tail_fwd[c128-t64-B256-stats]
  st_tail_kernel<256,16,4> / <256,32,4> full tail ............... test_tail_fwd[c256-t16-B2] [c256-t4-B4] [c256-t16-B512]
  head mode <256,16,8> <256,16,4> <256,32,4>, c 128 nine saves .. test_tail_fwd[c256-t16-B2-head] [c256-t16-B256-head]
                                                                  [c256-t16-B512-head] [c128-t64-B2-head]
  64-row tile declined for LDS -> 16 rows ....................... test_tail_fwd[c64-t4-B4096-n40]
  key split over 2 / 4 lanes, n_ctx 1 / 3 / 64 (empty lanes) .... test_tail_fwd[c64-t16-B2-n1] [-n3] [-n64] [c128-t4-B4-n1] [-n3]
  statistics slots: per slot row, other producer's columns ...... every -stats / -add / -store case
  tail forward refusals ......................................... test_tail_fwd_refusals
  st_head_kernel<64,16> <128,16> <128,32> <64,64> <128,64>,
    producer statistics + n1 s1 gn gn_stats ..................... test_head_fwd_train[...]
  st_head_kernel 16 rows: read-gn form .......................... test_head_fwd_read_gn[64] [128] [256]
  st_head_kernel 16 rows: self statistics (several images, the
    masked tail of the 8-row loop, several passes) .............. test_head_fwd_self_stats[...]
  head forward refusals ......................................... test_head_fwd_refusals
  st_tail_bwd_kernel<64,64,MF / VALU>, 1 and 4 tiles per image .. test_tail_bwd[c64-t64-B2-n28] [-n29] [c64-t256-B1-n28] [-n29]
  st_tail_bwd_kernel<128,32,MF / VALU>, 1 and 2 tiles ........... test_tail_bwd[c128-t32-B4-n24] [-n25] [c128-t64-B2-n24] [-n25]
  st_tail_bwd_kernel<128,64,MF / VALU> .......................... test_tail_bwd[c128-t64-B256-n20] [-n48] [-n64]
  padded keys (n_ctx % 4), MF 1 / 3 / 17, VALU 33 ............... test_tail_bwd[c64-t64-B2-n1] [-n3] [-n17] [-n33]
  tail backward refusals ........................................ test_tail_bwd_refusals
  encdiff_st_tail_bwd_tile against StPlan's copy ................ test_tail_bwd_tile_export
  st_head_bwd_kernel<64,32> <64,64> <128,32>, +- kv fold ........ test_head_bwd[...]
  forward -> backward layouts (s2 s3 lse2 f), per width ......... test_chained[64] [128] [256]

Measured on the MI355X: 70 cases, 5.7 s wall for the file; the slowest case 1.6 s (the first, which
loads the library), every other below 0.15 s.  Per stage over all cases -- largest floor (4 x |torch
fp32 - fp64|) / largest |out - ref| / largest fraction of the bound used.  A stored bf16 stage uses
all of its bound by construction (some element always rounds at half an ulp); the stages that carry
an unstored rounding through a contraction stay well inside their worst case; where a reference is
identically zero (n_ctx = 1: dS = 0, so d_q2, d_n2 and the LN2 partials vanish) the fraction is a
ratio of two rounding noises.
  forward head   gn_stats 5.2e-07 / 1.5e-07 / 0.21   gn 2.2e-06 / 1.6e-02 / 1.00   t0 1.4e-05 / 1.6e-02 / 1.00
                 s1 5.6e-07 / 2.1e-07 (fp32 rule)    n1 2.5e-06 / 1.6e-02 / 1.00   qkv 1.6e-05 / 1.7e-02 / 1.00
  forward tail   t1 6.7e-06 / 1.6e-02 / 1.00   s2 4.2e-07 / 1.4e-07   n2 3.0e-06 / 1.6e-02 / 1.00   q2 6.9e-06 / 1.6e-02 / 1.00
                 o2 4.6e-06 / 7.8e-03 / 1.00   lse2 2.9e-06 / 7.5e-07 / 0.11   t2 2.9e-06 / 3.1e-02 / 1.00   s3 3.6e-07 / 1.1e-07
                 n3 3.0e-06 / 1.6e-02 / 1.00   f 8.3e-06 / 1.6e-02 / 1.00   a 4.9e-06 / 3.1e-02 / 1.00   t3 1.8e-05 / 4.2e-02 / 1.00
                 out 1.1e-05 / 3.1e-02 / 1.00   slots 2.0e-04 / 5.7e-05 / 0.31
  backward tail  d_t3 5.6e-07 / 1.9e-03 / 1.00   d_f 6.2e-07 / 3.6e-03 / 1.00   d_t2 1.8e-06 / 3.4e-03 / 0.92
                 ln3_dg 6.1e-06 / 7.5e-03 / 0.61   ln3_db 6.9e-06 / 5.5e-03 / 0.46   d_q2 5.7e-07 / 1.8e-03 / 0.54
                 dk2 | dv2 1.5e-06 / 5.6e-03 / 0.78   kv_part 4.9e-07 / 1.2e-03 / 0.64   d_t1 2.5e-07 / 3.7e-03 / 0.98
                 ln2_dg 6.8e-07 / 2.6e-03 / 0.95   ln2_db 5.7e-07 / 2.6e-03 / 0.97   d_o1 6.9e-07 / 2.0e-03 / 1.00
  backward head  d_t0 1.2e-06 / 4.6e-03 / 0.89   ln1_dg 3.7e-06 / 1.1e-02 / 0.48   ln1_db 2.9e-06 / 9.0e-03 / 0.40
                 d_gn 9.2e-07 / 3.9e-03 / 1.00   kv fold: bitwise
"""
import math
from types import SimpleNamespace as NS

import pytest
import torch

import elementwise_restate as R
import st_restate as S
from test_gpu_elementwise import BF16, F32, F64, SENT, Guard, _gen, assert_f32_rule, dev, place, rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
GN_EPS, LN_EPS = 1e-6, 1e-5
STATS = {}  # stage -> [largest floor, largest error, largest error / bound]


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    S.StPlan.head_bwd(64, 64)  # refuses to run with a dispatch knob set in the environment
    from encdiff_amd import ops
    assert ops.ST_TAIL_STATS_ADD and not ops.ST_TAIL_R32_C64
    yield ops
    print("\nstage: largest floor / largest |out - ref| / largest fraction of the bound used")
    for k in sorted(STATS):
        print(f"  {k:10s} {STATS[k][0]:.2e} {STATS[k][1]:.2e} {STATS[k][2]:.3f}")


# ====================================================================== plumbing
def nan_guard(rows, cols):
    return Guard(rows, cols, F32, init=torch.full((rows, cols), NAN, device=dev), fill=NAN)


class Inputs:
    """Activations as the kernels get them: column views of wider buffers whose rows end in 8 NaN columns
    (several tensors side by side in one buffer, as k2 | v2); unchanged() proves no launch wrote any of them."""

    def __init__(self):
        self.bufs = []

    def rows(self, *xs):
        w = sum(x.shape[1] for x in xs)
        buf = torch.full((xs[0].shape[0], w + 8), NAN, dtype=xs[0].dtype, device=dev)
        views, c0 = [], 0
        for x in xs:
            buf[:, c0:c0 + x.shape[1]] = x
            views.append(buf[:, c0:c0 + x.shape[1]])
            c0 += x.shape[1]
        self.bufs.append((buf, buf.clone()))
        return views[0] if len(views) == 1 else views

    def keep(self, t):
        self.bufs.append((t, t.clone()))
        return t

    def unchanged(self):
        assert all(R.same_bits(a, b) for a, b in self.bufs), "an input buffer was written"


def bound(what, out, f, slack=0.0, store=True):
    """|out - ref64| <= slack + floor + (a bf16 store: half a bf16 ulp | fp32: 2^-22 |ref|) per element.
    f: dtype -> reference, or the pair (ref64, ref32)."""
    r64, r32 = f if isinstance(f, tuple) else (f(F64), f(F32))
    assert out.shape == r64.shape, (what, out.shape, r64.shape)
    floor = R.floor_of(r32, r64)
    s = torch.as_tensor(slack, dtype=F64, device=dev) + floor
    tol = S.bf16_store_tol(r64, s) if store else S.f32_tol(r64, s)
    assert not torch.isnan(out).any(), f"{what}: NaN (unwritten or poisoned) in the output"
    err = (out.double() - r64).abs()
    ex = err - tol
    i = int(ex.argmax())
    used = (err / tol.clamp_min(1e-300)).max().item()
    st = STATS.setdefault(what.split()[-1], [0.0, 0.0, 0.0])
    st[0], st[1], st[2] = max(st[0], floor), max(st[1], err.max().item()), max(st[2], used)
    print(f"{what}: floor {floor:.3e} max|out-ref| {err.max().item():.3e} bound used {used:.3f}")
    idx, k = [], i
    for n in reversed(ex.shape):
        idx.insert(0, k % n)
        k //= n
    idx = tuple(idx)
    assert ex.flatten()[i].item() <= 0, (f"{what}: element {idx} = {out[idx].item()!r} vs {r64[idx].item()!r} exceeds "
                                         f"the bound {tol[idx].item():.3e} by {ex.flatten()[i].item():.3e}")


def f32_rule(what, out, f):
    """fp32 statistics: the fp32 rule of the step-kernel tests, floor + 2^-22 |ref|"""
    r64, r32 = f(F64), f(F32)
    assert not torch.isnan(out).any(), f"{what}: NaN (unwritten or poisoned) in the output"
    assert_f32_rule(out, r64, r32, what)
    st = STATS.setdefault(what.split()[-1], [0.0, 0.0, 0.0])
    st[0], st[1] = max(st[0], R.floor_of(r32, r64)), max(st[1], (out.double() - r64).abs().max().item())


def carried(f):
    """(unrounded fp64 value, half a bf16 ulp of it widened by its own floor) of an operand the kernel
    rounds without storing it"""
    r64 = f(F64)
    return r64, S.half_ulp(r64.abs() + R.floor_of(f(F32), r64))


def twice(run):
    """Run a launch twice into fresh Guards; both must agree bitwise.  run() -> dict name -> Guard."""
    a, b = run(), run()
    for k in a:
        assert R.same_bits(a[k].buf, b[k].buf), f"{k}: two launches on the same inputs differ bitwise"
    return NS(**{k: g.view for k, g in a.items()}), a


def weights(g, c, strided=True):
    """The block's parameters: bf16 GEMM weights [out][in] (strided views), fp32 biases / affines"""
    w = lambda o, i: place(rnd(g, o, i, scale=i ** -0.5, dtype=BF16), strided)
    v = lambda n, base=0.0: (base + 0.1 * torch.randn(n, generator=g)).to(dev)
    return {"in": w(c, c), "b_in": v(c), "g1": v(c, 1.0), "be1": v(c), "qkv": w(3 * c, c), "gn_g": v(c, 1.0),
            "gn_b": v(c), "out1": w(c, c), "b_out1": v(c), "g2": v(c, 1.0), "be2": v(c), "q2": w(c, c),
            "out2": w(c, c), "b_out2": v(c), "g3": v(c, 1.0), "be3": v(c), "ff1": w(8 * c, c), "b_ff1": v(8 * c),
            "ff2": w(c, 4 * c), "b_ff2": v(c), "po": w(c, c), "b_po": v(c)}


def transposed(W):
    """The dense transposed copies the backward kernels read ([in][out])"""
    return {k: W[k].t().contiguous() for k in ("po", "ff2", "ff1", "out2", "q2", "out1", "qkv", "in")}


def expect(p, **want):
    assert p.rc == S.OK, f"launch plan changed: declined ({p.rc})"
    for k, v in want.items():
        assert getattr(p, k) == v, f"launch plan changed: {k} = {getattr(p, k)}, this case needs {v}"


# ====================================================================== forward tail
class TailIn:
    def __init__(self, c, tokens, B, nctx, seed):
        g = _gen(seed)
        self.c, self.tokens, self.B, self.nctx, self.rows = c, tokens, B, nctx, B * tokens
        self.inp = Inputs()
        r = lambda n, s=1.0: rnd(g, n, c, scale=s, dtype=BF16)
        self.o1, self.t0, self.x = (self.inp.rows(r(self.rows)) for _ in range(3))
        self.k2, self.v2 = self.inp.rows(r(B * nctx), r(B * nctx))
        self.W = weights(g, c)


def run_tail_fwd(O, t, saves, stats=False, head=False):
    c, rows, B = t.c, t.rows, t.B

    def run():
        o = {"out": Guard(rows, c, BF16, strided=True)}
        names = []
        if saves:
            names = ["t1", "n2", "q2", "o2", "t2", "n3"] + ([] if head else ["t3"])
        elif head:
            names = ["t2", "n3"]
        for k in names:
            o[k] = Guard(rows, c, BF16, strided=True)
        if saves:
            if not head:
                o["f"], o["a"] = Guard(rows, 8 * c, BF16), Guard(rows, 4 * c, BF16)  # dense: the kernel's layout
            o["s2"], o["s3"], o["lse2"] = nan_guard(rows, 2), nan_guard(rows, 2), nan_guard(B * 8, t.tokens)
        if stats:
            o["slots"] = Guard(2 * (rows // 64), 2 * c, F32, strided=True,
                               init=torch.full((2 * (rows // 64), 2 * c), 7.25, device=dev))
        sv = {k: o[k].view for k in o if k not in ("out", "slots")} if saves else None
        ok = O.st_tail_fwd(t.o1, t.t0, t.x, t.k2, t.v2, t.W, o["out"].view, rows, c, t.tokens, 8, t.nctx, LN_EPS,
                           save=sv, gn_stats=o["slots"].view if stats else None,
                           head=(o["t2"].view, o["n3"].view) if head else None)
        assert ok, f"declined: {getattr(O.st_tail_fwd, 'declined', None)}"
        torch.cuda.synchronize()
        for g in o.values():
            g.check()
        return o
    return twice(run)


def check_tail_fwd(t, o, what, head=False, stats=False, spl=1):
    W, c, B = t.W, t.c, t.B
    bound(what + " t1", o.t1, lambda d: S.lin(t.o1, W["out1"], W["b_out1"], t.t0, d))
    f32_rule(what + " s2", o.s2, lambda d: S.ln_stats(o.t1, LN_EPS, d))
    bound(what + " n2", o.n2, lambda d: S.ln_apply(o.t1, o.s2, W["g2"], W["be2"], d))
    bound(what + " q2", o.q2, lambda d: S.lin(o.n2, W["q2"], dt=d))
    a64, a32 = (S.cross_attn(o.q2, t.k2, t.v2, B, t.tokens, t.nctx, d) for d in (F64, F32))
    # p = exp(s - m) with m the lane's running maximum (|s - m| <= |s - lse| + log n_ctx), one further
    # exp per level of the SPL-lane merge; numerator and normaliser each carry them
    nexp = 1 + int(math.log2(spl))
    eps = S.exp_rel_of(a64.xmax + math.log(t.nctx))
    bound(what + " o2", o.o2, (a64.o, a32.o), slack=2 * nexp * eps * a64.abs_o)
    # lse = m + log(l): l carries the exps' relative error; the fast log is v_log_f32 (1 ulp of
    # log2 l <= 6) times ln 2
    bound(what + " lse2", o.lse2, (a64.lse, a32.lse), slack=nexp * eps + 2.0 ** -21, store=False)
    bound(what + " t2", o.t2, lambda d: S.lin(o.o2, W["out2"], W["b_out2"], o.t1, d), slack=S.half_ulp(o.t1.double()))
    f32_rule(what + " s3", o.s3, lambda d: S.ln_stats(o.t2, LN_EPS, d))
    bound(what + " n3", o.n3, lambda d: S.ln_apply(o.t2, o.s3, W["g3"], W["be3"], d))
    if head:
        assert (o.out == SENT).all(), "head mode wrote out"
        return
    bound(what + " f", o.f, lambda d: S.lin(o.n3, W["ff1"], W["b_ff1"], dt=d))
    fv, fg = o.f[:, :4 * c].double(), o.f[:, 4 * c:].double()
    bound(what + " a", o.a, lambda d: S.geglu(o.f, d), slack=fv.abs() * S.gelu_slack(fg))
    bound(what + " t3", o.t3, lambda d: S.lin(o.a, W["ff2"], W["b_ff2"], o.t2, d), slack=S.half_ulp(o.t2.double()))
    bound(what + " out", o.out, lambda d: S.lin(o.t3, W["po"], W["b_po"], t.x, d))
    if stats:
        # each slot row: the sum / the sum of squares of the STORED out of its 64-row segment
        bound(what + " slots", o.slots[:, :c], lambda d: S.gn_sums(o.out, d), store=False)
        assert (o.slots[:, c:] == 7.25).all(), "the concat's other producer's statistics columns were written"


# id: (c, tokens, B, n_ctx, form, expected plan)
TAIL_FWD = {
    "c64-t256-B1": (64, 256, 1, 20, "", dict(tile=16, waves=4, nimg=1, spl=2)),
    "c64-t16-B2": (64, 16, 2, 20, "", dict(tile=16, waves=4, nimg=1, spl=2)),
    "c64-t4-B8": (64, 4, 8, 20, "", dict(tile=16, waves=4, nimg=4, grid=2)),
    "c64-t64-B2-stats": (64, 64, 2, 20, "stats", dict(tile=64, waves=4, nimg=1, spl=1)),
    "c64-t16-B8-stats": (64, 16, 8, 20, "stats", dict(tile=64, waves=4, nimg=4, grid=2)),
    "c64-t256-B64": (64, 256, 64, 20, "", dict(tile=64, waves=4, nimg=1, grid=256)),
    "c64-t64-B2-r32add": (64, 64, 2, 20, "r32add", dict(tile=32, waves=4, grid=4)),
    "c128-t64-B2": (128, 64, 2, 20, "", dict(tile=16, waves=8, nimg=1, spl=4)),
    "c128-t4-B4": (128, 4, 4, 20, "", dict(tile=16, waves=8, nimg=4, grid=1)),
    "c128-t64-B2-add": (128, 64, 2, 20, "stats", dict(tile=32, waves=8, grid=4)),
    "c128-t64-B128-add": (128, 64, 128, 20, "stats", dict(tile=32, waves=4, grid=256)),
    "c128-t64-B2-store": (128, 64, 2, 20, "store", dict(tile=64, waves=8, grid=2)),
    "c128-t64-B256-stats": (128, 64, 256, 20, "stats", dict(tile=64, waves=4, grid=256)),
    "c256-t16-B2": (256, 16, 2, 20, "", dict(tile=16, waves=4, nimg=1, spl=2)),
    "c256-t4-B4": (256, 4, 4, 20, "", dict(tile=16, waves=4, nimg=4)),
    "c256-t16-B512": (256, 16, 512, 20, "", dict(tile=32, waves=4, nimg=2, grid=256)),
    "c256-t16-B2-head": (256, 16, 2, 20, "head", dict(tile=16, waves=8, spl=4)),
    "c256-t16-B256-head": (256, 16, 256, 20, "head", dict(tile=16, waves=4, grid=256)),
    "c256-t16-B512-head": (256, 16, 512, 20, "head", dict(tile=32, waves=4, grid=256)),
    "c128-t64-B2-head": (128, 64, 2, 20, "head", dict(tile=16, waves=8)),
    "c64-t4-B4096-n40": (64, 4, 4096, 40, "", dict(tile=16, waves=4, nimg=4, grid=1024)),
    "c64-t16-B2-n1": (64, 16, 2, 1, "", dict(tile=16, spl=2)),
    "c64-t16-B2-n3": (64, 16, 2, 3, "", dict(tile=16, spl=2)),
    "c64-t16-B2-n64": (64, 16, 2, 64, "", dict(tile=16, spl=2)),
    "c128-t4-B4-n1": (128, 4, 4, 1, "", dict(tile=16, waves=8, spl=4, nimg=4)),
    "c128-t4-B4-n3": (128, 4, 4, 3, "", dict(tile=16, waves=8, spl=4, nimg=4)),
}


@pytest.mark.parametrize("name", list(TAIL_FWD))
def test_tail_fwd(O, name, monkeypatch):
    """The training forward (all saves) stage by stage, then the inference launch bit-identical to it.
    Catches: a wave's 16 columns of one GEMM or GEGLU chunk shifted; a row group of a tile skipped; an
    image of a multi-image tile reading another image's K / V; lse2 at the wrong token; empty key
    lanes merged as non-zeros; a statistics slot of the wrong segment, rows swapped, or the other
    producer's columns touched; saves at the wrong leading dimension."""
    c, tokens, B, nctx, form, want = TAIL_FWD[name]
    if form == "r32add":
        monkeypatch.setattr(O, "ST_TAIL_R32_C64", True)
    if form == "store":
        monkeypatch.setattr(O, "ST_TAIL_STATS_ADD", False)
    stats, head = form in ("stats", "r32add", "store"), form == "head"
    rows = B * tokens
    add = stats and S.StPlan.stats_add(c, rows, O.ST_TAIL_R32_C64, O.ST_TAIL_STATS_ADD)
    plan = S.StPlan.tail_fwd(c, rows, tokens, nctx, gn_stats=stats, add=add, head=head)
    expect(plan, **want)
    if name.endswith("-add") or form == "r32add":
        assert add
    t = TailIn(c, tokens, B, nctx, seed=sum(map(ord, name)))
    o, g = run_tail_fwd(O, t, True, stats, head)
    check_tail_fwd(t, o, name, head, stats, plan.spl)
    oi, gi = run_tail_fwd(O, t, False, stats, head)
    for k in (("t2", "n3") if head else ("out",) + (("slots",) if stats else ())):
        assert R.same_bits(getattr(oi, k), getattr(o, k)), f"{k}: the inference launch differs from the training launch"
    t.inp.unchanged()


def test_tail_fwd_refusals(O):
    t = TailIn(256, 16, 4, 20, 5)
    out = Guard(96, 256, BF16, strided=True)
    slots = nan_guard(2, 512)
    call = lambda t, **kw: O.st_tail_fwd(t.o1, t.t0, t.x, t.k2, t.v2, t.W, out.view[:t.rows, :t.c], t.rows, t.c,
                                         t.tokens, 8, t.nctx, LN_EPS, **kw)
    assert S.StPlan.tail_fwd(256, 64, 16, 20, gn_stats=True).rc == S.ERR_SHAPE
    assert not call(t, gn_stats=slots.view)            # producer statistics at c = 256
    t = TailIn(64, 16, 6, 20, 6)                        # 96 rows: no whole 64-row segments
    assert S.StPlan.tail_fwd(64, 96, 16, 20, gn_stats=True).rc == S.ERR_SHAPE
    assert not call(t, gn_stats=slots.view)
    torch.cuda.synchronize()
    out.check()
    slots.check()
    assert torch.isnan(slots.view).all() and (out.view == SENT).all()


# ====================================================================== forward head
class HeadIn:
    def __init__(self, c, tokens, B, seed):
        g = _gen(seed)
        self.c, self.tokens, self.B, self.rows = c, tokens, B, B * tokens
        self.inp = Inputs()
        self.x = self.inp.rows(rnd(g, self.rows, c, dtype=BF16) + 0.25)
        self.W = weights(g, c)


def run_head_fwd(O, h, form, train):
    """form: 'producer' (segment sums -> gn, gn_stats written), 'read' (gn given), 'self'"""
    c, rows, W = h.c, h.rows, h.W
    sums = gn_in = None
    if form == "producer":
        sums = h.inp.rows(S.gn_sums(h.x, F32))
    if form == "read":
        st = S.gn_stats_from_x(h.x, h.B, h.tokens, c, GN_EPS, F32)
        gn_in = h.inp.rows(S.gn_apply(h.x, st, W["gn_g"], W["gn_b"], h.B, h.tokens, F32).to(BF16))

    def run():
        o = {"t0": Guard(rows, c, BF16, strided=True), "qkv": Guard(rows, 3 * c, BF16, strided=True)}
        if form != "read":
            o["gn"] = Guard(rows, c, BF16, strided=True)
        if form == "producer":
            o["gn_stats"] = nan_guard(h.B * 32, 2)
        if train:
            o["n1"], o["s1"] = Guard(rows, c, BF16, strided=True), nan_guard(rows, 2)
        ok = O.st_head_fwd(h.x, gn_in if form == "read" else o["gn"].view, W["in"], W["b_in"], W["g1"], W["be1"],
                           W["qkv"], o["t0"].view, o["qkv"].view, rows, c, h.tokens, GN_EPS, LN_EPS, in_stats=sums,
                           gn_gamma=W["gn_g"], gn_beta=W["gn_b"], gn_stats=o["gn_stats"].view if form == "producer" else None,
                           n1=o["n1"].view if train else None, s1=o["s1"].view if train else None,
                           self_stats=form == "self")
        assert ok, "declined"
        torch.cuda.synchronize()
        for g in o.values():
            g.check()
        return o
    o, g = twice(run)
    o.sums, o.gn_in = sums, gn_in
    return o


def check_head_fwd(h, o, what, form, train):
    W, c, B = h.W, h.c, h.B
    gn_slack = 0.0
    if form == "producer":
        bound(what + " gn_stats", o.gn_stats,
              lambda d: S.gn_stats_from_sums(o.sums, B, h.tokens, c, GN_EPS, d).reshape(B * 32, 2), store=False)
        bound(what + " gn", o.gn, lambda d: S.gn_apply(h.x, o.gn_stats.reshape(B, 32, 2), W["gn_g"], W["gn_b"], B, h.tokens, d))
        gn = lambda d: o.gn
    elif form == "read":
        gn = lambda d: o.gn_in
    else:  # gn is an operand only: unrounded in the reference, its half-ulp carried through proj_in
        assert (o.gn == SENT).all(), "the self-statistics form wrote gn"
        gn = lambda d: S.gn_apply(h.x, S.gn_stats_from_x(h.x, B, h.tokens, c, GN_EPS, d), W["gn_g"], W["gn_b"], B, h.tokens, d)
        gn_slack = carried(gn)[1] @ W["in"].double().abs().t()
    bound(what + " t0", o.t0, lambda d: S.lin(gn(d), W["in"], W["b_in"], dt=d), slack=gn_slack)
    if train:
        f32_rule(what + " s1", o.s1, lambda d: S.ln_stats(o.t0, LN_EPS, d))
        bound(what + " n1", o.n1, lambda d: S.ln_apply(o.t0, o.s1, W["g1"], W["be1"], d))
        bound(what + " qkv", o.qkv, lambda d: S.lin(o.n1, W["qkv"], dt=d))
    else:
        n1 = lambda d: S.ln_apply(o.t0, S.ln_stats(o.t0, LN_EPS, d), W["g1"], W["be1"], d)
        bound(what + " qkv", o.qkv, lambda d: S.lin(n1(d), W["qkv"], dt=d),
              slack=carried(n1)[1] @ W["qkv"].double().abs().t())


@pytest.mark.parametrize("c,tokens,B,tile", [(64, 64, 2, 16), (128, 64, 2, 16), (128, 64, 128, 32), (64, 256, 64, 64),
                                             (128, 64, 256, 64)])
def test_head_fwd_train(O, c, tokens, B, tile):
    """Producer statistics with n1, s1, gn and gn_stats written, on every tile.  Catches: a segment's
    sums taken from the neighbouring image; mean / rstd swapped or written by the wrong tile; t0 saved
    unrounded while LN1 reads the rounded row (or the reverse); a q / k / v column block misplaced."""
    what = f"head c{c} t{tokens} B{B}"
    expect(S.StPlan.head_fwd(c, B * tokens, tokens, in_stats=True, n1=True), tile=tile, waves=4, nimg=1)
    h = HeadIn(c, tokens, B, seed=c + tokens + B)
    o = run_head_fwd(O, h, "producer", True)
    check_head_fwd(h, o, what, "producer", True)
    oi = run_head_fwd(O, h, "producer", False)  # no n1 / s1: t0 by the inference store, the same bits
    for k in ("t0", "qkv", "gn", "gn_stats"):
        assert R.same_bits(getattr(oi, k), getattr(o, k)), k
    h.inp.unchanged()


@pytest.mark.parametrize("c", [64, 128, 256])
def test_head_fwd_read_gn(O, c):
    expect(S.StPlan.head_fwd(c, 32, 16), tile=16, waves=8 if c == 256 else 4)
    h = HeadIn(c, 16, 2, seed=c + 1)
    for train in ((True, False) if c < 256 else (False,)):
        o = run_head_fwd(O, h, "read", train)
        check_head_fwd(h, o, f"head-read c{c} train{int(train)}", "read", train)
    h.inp.unchanged()


@pytest.mark.parametrize("c,tokens,B", [(64, 4, 8), (64, 16, 2), (128, 4, 4), (128, 16, 2), (256, 4, 4), (256, 16, 2),
                                        (64, 144, 1), (256, 1024, 1)])
def test_head_fwd_self_stats(O, c, tokens, B):
    """The kernel's own GroupNorm statistics: several images per tile (tokens 4: four), the masked tail
    of the 8-row unrolled loop (tokens 144 at c 64: 32 token lanes, 144 = 4 x 32 + 16), several passes
    (tokens 1024 at c 256).  Catches: an image's statistics from its neighbour's rows; rows past the
    image's last token read; a pass skipped."""
    p = S.StPlan.head_fwd(c, B * tokens, tokens, self_stats=True)
    expect(p, tile=16, waves=8 if c == 256 else 4, nimg=max(1, 16 // tokens))
    h = HeadIn(c, tokens, B, seed=3 * c + tokens)
    o = run_head_fwd(O, h, "self", False)
    check_head_fwd(h, o, f"head-self c{c} t{tokens}", "self", False)
    h.inp.unchanged()


def test_head_fwd_refusals(O):
    h = HeadIn(256, 16, 2, 9)
    W = h.W
    t0, qkv, gn, n1 = (Guard(64, 3 * 256 if k == 1 else 256, BF16, strided=True) for k in range(4))
    s1 = nan_guard(64, 2)
    call = lambda h, rows, tokens, **kw: O.st_head_fwd(
        h.x[:rows], gn.view[:rows, :h.c], W["in"][:h.c, :h.c], W["b_in"], W["g1"], W["be1"], W["qkv"][:3 * h.c, :h.c],
        t0.view[:rows, :h.c], qkv.view[:rows, :3 * h.c], rows, h.c, tokens, GN_EPS, LN_EPS, gn_gamma=W["gn_g"],
        gn_beta=W["gn_b"], **kw)
    assert S.StPlan.head_fwd(256, 32, 16, n1=True).rc == S.ERR_SHAPE
    assert not call(h, 32, 16, n1=n1.view[:32], s1=s1.view[:32], self_stats=True)        # c 256 with n1
    assert S.StPlan.head_fwd(256, 8, 4, self_stats=True).rc == S.ERR_SHAPE
    assert not call(h, 8, 4, self_stats=True)                                            # rows % 16 != 0
    h64 = HeadIn(64, 16, 4, 10)
    W = h64.W
    assert S.StPlan.head_fwd(64, 64, 16, in_stats=True).rc == S.ERR_SHAPE
    sums = S.gn_sums(h64.x, F32)
    assert not call(h64, 64, 16, in_stats=sums, gn_stats=s1.view[:32])                   # tokens % 64 with producer sums
    torch.cuda.synchronize()
    for g in (t0, qkv, gn, n1, s1):
        g.check()
        assert (g.view == SENT).all() if g.view.dtype == BF16 else torch.isnan(g.view).all()


# ====================================================================== backward tail
def ref_saves(t):
    """The forward's saves for a backward-only case: the restated chain with the kernel's roundings,
    in fp32, stored as the forward stores them"""
    r = S.tail_fwd(t.o1, t.t0, t.x, t.k2, t.v2, t.W, t.B, t.tokens, t.nctx, LN_EPS, True, F32)
    inp = t.inp
    t2, t1, q2, o2 = (inp.rows(getattr(r, k).to(BF16)) for k in ("t2", "t1", "q2", "o2"))
    return NS(f=inp.rows(r.f.to(BF16)), t2=t2, t1=t1, q2=q2, o2=o2, s3=inp.keep(r.s3.contiguous()),
              s2=inp.keep(r.s2.contiguous()), lse2=inp.keep(r.lse2.contiguous()))


def run_tail_bwd(O, t, sv, dy, wt, plan, extra_parts=3):
    c, rows, B, nctx = t.c, t.rows, t.B, t.nctx
    tiles = plan.grid

    def run():
        o = {k: Guard(rows, c, BF16, strided=True) for k in ("d_t3", "d_t2", "d_q2", "d_t1", "d_o1")}
        o["d_f"] = Guard(rows, 8 * c, BF16, strided=True)
        o["pm"] = Guard(tiles + extra_parts, 4 * c, F32, strided=True,
                        init=torch.full((tiles + extra_parts, 4 * c), NAN, device=dev), fill=NAN)
        o["dkv"] = Guard(B * nctx, 2 * c, BF16, strided=True)
        o["kv_part"] = nan_guard(tiles * nctx, 2 * c)
        pm = o["pm"].view
        ok = O.st_tail_bwd(dy, vars(sv), wt, t.W["g3"], t.W["g2"], t.k2, t.v2, {k: o[k].view for k in o if k[0] == "d" and k != "dkv"},
                           (pm[:, :c], pm[:, c:2 * c]), (pm[:, 2 * c:3 * c], pm[:, 3 * c:]),
                           o["dkv"].view[:, :c], o["dkv"].view[:, c:], rows, c, t.tokens, 8, nctx,
                           kv_part=o["kv_part"].view)
        assert ok, "declined"
        torch.cuda.synchronize()
        for g in o.values():
            g.check()
        return o
    return twice(run)


def check_tail_bwd(t, sv, dy, o, plan, what):
    W, c, B, nctx, R_ = t.W, t.c, t.B, t.nctx, plan.tile
    tiles = plan.grid
    bound(what + " d_t3", o.d_t3, lambda d: S.lin_bwd(dy, W["po"], d))
    # d_a is rounded and not stored: kept unrounded here, its half-ulp h_a scaled by the GEGLU factors
    d_a = lambda d: S.lin_bwd(o.d_t3, W["ff2"], d)
    a64, h_a = carried(d_a)
    fv, fg = sv.f[:, :4 * c].double(), sv.f[:, 4 * c:].double()
    slack = torch.cat([h_a * S.gelu(fg).abs() + a64.abs() * S.gelu_slack(fg),
                       h_a * (fv * S.gelu_grad(fg)).abs() + (a64 * fv).abs() * S.gelu_grad_slack(fg)], 1)
    bound(what + " d_f", o.d_f, lambda d: S.geglu_bwd(sv.f, d_a(d), d), slack=slack)
    d_n3 = lambda d: S.lin_bwd(o.d_f, W["ff1"], d)
    h3 = carried(d_n3)[1]
    bound(what + " d_t2", o.d_t2, lambda d: o.d_t3.to(d) + S.ln_bwd(sv.t2, sv.s3, W["g3"], d_n3(d), d),
          slack=S.half_ulp(o.d_t3.double()) + S.ln_bwd_abs(sv.t2, sv.s3, W["g3"], h3))
    pm = o.pm
    assert torch.isnan(pm[tiles:]).all(), "a LayerNorm partial row past the launched tiles was written"
    # every tile's partial row against the sums over ITS rows (h3 / h2: the rounded d_n3 / d_n2)
    for i, nm in enumerate(("ln3_dg", "ln3_db")):
        bound(what + " " + nm, pm[:tiles, i * c:(i + 1) * c], lambda d: S.ln_partials(sv.t2, sv.s3, d_n3(d), R_, d)[i],
              slack=S.ln_partials_abs(sv.t2, sv.s3, h3, R_)[i], store=False)
    d_o2 = lambda d: S.lin_bwd(o.d_t2, W["out2"], d)
    o64, h_o = carried(d_o2)
    eps = S.exp_rel_of(S.cross_attn(sv.q2, t.k2, t.v2, B, t.tokens, nctx, F64).xmax + 1e-3)
    at = S.cross_attn_bwd(sv.q2, t.k2, t.v2, sv.o2, sv.lse2, o64, B, t.tokens, nctx, R_, F64, h_do=h_o, mf=plan.mf,
                          exp_rel=eps)
    at32 = S.cross_attn_bwd(sv.q2, t.k2, t.v2, sv.o2, sv.lse2, d_o2(F32), B, t.tokens, nctx, R_, F32)
    bound(what + " d_q2", o.d_q2, (at.dq, at32.dq), slack=at.s_dq)
    if plan.tpi == 1:
        assert torch.isnan(o.kv_part).all(), "one tile per image wrote a partial slab"
        bound(what + " dkv", o.dkv, (at.dkv.reshape(B * nctx, 2 * c), at32.dkv.reshape(B * nctx, 2 * c)),
              slack=at.s_dkv.reshape(B * nctx, 2 * c))
    else:  # each tile's fp32 slab on its own
        assert (o.dkv == SENT).all(), "several tiles per image wrote dk2 / dv2 (the head backward folds the slabs)"
        bound(what + " kv_part", o.kv_part.reshape(tiles, nctx, 2 * c), (at.dkv, at32.dkv), slack=at.s_dkv, store=False)
    d_n2 = lambda d: S.lin_bwd(o.d_q2, W["q2"], d)
    h2 = carried(d_n2)[1]
    bound(what + " d_t1", o.d_t1, lambda d: o.d_t2.to(d) + S.ln_bwd(sv.t1, sv.s2, W["g2"], d_n2(d), d),
          slack=S.half_ulp(o.d_t2.double()) + S.ln_bwd_abs(sv.t1, sv.s2, W["g2"], h2))
    for i, nm in enumerate(("ln2_dg", "ln2_db")):
        bound(what + " " + nm, pm[:tiles, (2 + i) * c:(3 + i) * c], lambda d: S.ln_partials(sv.t1, sv.s2, d_n2(d), R_, d)[i],
              slack=S.ln_partials_abs(sv.t1, sv.s2, h2, R_)[i], store=False)
    bound(what + " d_o1", o.d_o1, lambda d: S.lin_bwd(o.d_t1, W["out1"], d))


MF64, MF128_32, MF128_64 = S.mf_last(64, 64), S.mf_last(128, 32), S.mf_last(128, 64)
# id: (c, tokens, B, n_ctx, expected tile, MF form, tiles per image)
TAIL_BWD = {}
for _n, _mf in ((MF64, True), (MF64 + 1, False)):
    TAIL_BWD[f"c64-t64-B2-n{_n}"] = (64, 64, 2, _n, 64, _mf, 1)
    TAIL_BWD[f"c64-t256-B1-n{_n}"] = (64, 256, 1, _n, 64, _mf, 4)
for _n, _mf in ((MF128_32, True), (MF128_32 + 1, False)):
    TAIL_BWD[f"c128-t32-B4-n{_n}"] = (128, 32, 4, _n, 32, _mf, 1)
    TAIL_BWD[f"c128-t64-B2-n{_n}"] = (128, 64, 2, _n, 32, _mf, 2)
for _n, _mf in ((20, True), (MF128_64, True), (64, False)):
    TAIL_BWD[f"c128-t64-B256-n{_n}"] = (128, 64, 256, _n, 64, _mf, 1)
for _n, _mf in ((1, True), (3, True), (17, True), (33, False)):
    TAIL_BWD[f"c64-t64-B2-n{_n}"] = (64, 64, 2, _n, 64, _mf, 1)


@pytest.mark.parametrize("name", list(TAIL_BWD))
def test_tail_bwd(O, name):
    """Both key-gradient forms on every tile, at the derived boundary n_ctx (st_restate.mf_last: 28 / 24 /
    48), one and several tiles per image, padded keys.  Catches: a wave's columns of one input-gradient
    GEMM or GEGLU chunk shifted; d_a / d_n3 / d_o2 / d_n2 used unrounded or rounded twice; a LayerNorm
    partial row written by the wrong tile or summed over another tile's rows; a padded key
    (n_ctx % 4 != 0) leaking into dK / dV or the last real key dropped; a slab of the wrong tile."""
    c, tokens, B, nctx, tile, mf, tpi = TAIL_BWD[name]
    rows = B * tokens
    plan = S.StPlan.tail_bwd(c, rows, tokens, nctx, part_rows=rows // tile + 3)
    expect(plan, tile=tile, mf=mf, tpi=tpi)
    assert O.st_tail_bwd_tile(c, rows, tokens) == tile == S.StPlan.tail_bwd_tile(c, rows, tokens)
    t = TailIn(c, tokens, B, nctx, seed=sum(map(ord, name)))
    sv = ref_saves(t)
    dy = t.inp.rows(rnd(_gen(7), rows, c, scale=0.1, dtype=BF16))
    o, g = run_tail_bwd(O, t, sv, dy, transposed(t.W), plan)
    check_tail_bwd(t, sv, dy, o, plan, name)
    t.inp.unchanged()


def test_tail_bwd_tile_export(O):
    """encdiff_st_tail_bwd_tile, the one dispatch decision the library exports, against StPlan's copy"""
    for c in (64, 128):
        for tokens in (16, 32, 64, 96, 256, 1024):
            for B in (1, 2, 127, 128, 255, 256, 257, 512):
                assert O.st_tail_bwd_tile(c, B * tokens, tokens) == S.StPlan.tail_bwd_tile(c, B * tokens, tokens), (c, tokens, B)


def test_tail_bwd_refusals(O):
    from encdiff_amd._lib import HipError
    t = TailIn(64, 16, 4, 20, 11)
    assert S.StPlan.tail_bwd(64, 64, 16, 20).rc == S.ERR_SHAPE
    sv = ref_saves(t)
    dy = t.inp.rows(rnd(_gen(8), t.rows, 64, scale=0.1, dtype=BF16))
    wt = transposed(t.W)
    outs = {k: Guard(256, 64, BF16, strided=True) for k in ("d_t3", "d_t2", "d_q2", "d_t1", "d_o1")}
    outs["d_f"] = Guard(256, 512, BF16, strided=True)
    pm, dkv, kvp = nan_guard(8, 256), Guard(20, 128, BF16, strided=True), nan_guard(4 * 20, 128)

    def call(t, sv, dy, parts, kv_part):
        p, r = pm.view[:parts], t.rows
        return O.st_tail_bwd(dy, vars(sv), wt, t.W["g3"], t.W["g2"], t.k2, t.v2, {k: g.view[:r] for k, g in outs.items()},
                             (p[:, :64], p[:, 64:128]), (p[:, 128:192], p[:, 192:]), dkv.view[:, :64], dkv.view[:, 64:],
                             r, 64, t.tokens, 8, 20, kv_part=kv_part)
    assert not call(t, sv, dy, 8, kvp.view)                     # tokens 16: no whole 64-row tile
    t = TailIn(64, 256, 1, 20, 12)
    sv = ref_saves(t)
    dy = t.inp.rows(rnd(_gen(8), 256, 64, scale=0.1, dtype=BF16))
    wt = transposed(t.W)
    assert S.StPlan.tail_bwd(64, 256, 256, 20, part_rows=3).rc == S.ERR_SHAPE
    assert not call(t, sv, dy, 3, kvp.view)                     # part_rows below the four launched tiles
    with pytest.raises(HipError):                               # four tiles per image and no kv_part
        call(t, sv, dy, 8, None)
    torch.cuda.synchronize()
    for g in list(outs.values()) + [pm, dkv, kvp]:
        g.check()
        assert (g.view == SENT).all() if g.view.dtype == BF16 else torch.isnan(g.view).all()


# ====================================================================== backward head
def run_head_bwd(O, W, wt, inp, d_qkv, d_t1, t0, s1, rows, c, plan, kv=None):
    tiles = plan.grid

    def run():
        o = {"d_t0": Guard(rows, c, BF16, strided=True), "d_gn": Guard(rows, c, BF16, strided=True),
             "pm": Guard(tiles + 2, 2 * c, F32, strided=True, init=torch.full((tiles + 2, 2 * c), NAN, device=dev), fill=NAN)}
        kva = None
        if kv is not None:
            kv_part, tpi, nctx, B = kv
            o["dkv"] = Guard(B * nctx, 2 * c, BF16, strided=True)
            kva = (kv_part, tpi, nctx, B, o["dkv"].view[:, :c], o["dkv"].view[:, c:])
        pm = o["pm"].view
        assert O.st_head_bwd(d_qkv, d_t1, t0, s1, W["g1"], wt["qkv"], wt["in"], o["d_t0"].view, o["d_gn"].view,
                             (pm[:, :c], pm[:, c:]), rows, c, kv=kva), "declined"
        torch.cuda.synchronize()
        for g in o.values():
            g.check()
        return o
    return twice(run)


def check_head_bwd(W, d_qkv, d_t1, t0, s1, o, plan, what, kv=None):
    c, tiles, R_ = plan.c, plan.grid, plan.tile
    d_n1 = lambda d: S.lin_bwd(d_qkv, W["qkv"], d)
    h1 = carried(d_n1)[1]
    bound(what + " d_t0", o.d_t0, lambda d: d_t1.to(d) + S.ln_bwd(t0, s1, W["g1"], d_n1(d), d),
          slack=S.ln_bwd_abs(t0, s1, W["g1"], h1))
    assert torch.isnan(o.pm[tiles:]).all(), "a LayerNorm partial row past the launched tiles was written"
    for i, nm in enumerate(("ln1_dg", "ln1_db")):
        bound(what + " " + nm, o.pm[:tiles, i * c:(i + 1) * c], lambda d: S.ln_partials(t0, s1, d_n1(d), R_, d)[i],
              slack=S.ln_partials_abs(t0, s1, h1, R_)[i], store=False)
    bound(what + " d_gn", o.d_gn, lambda d: S.lin_bwd(o.d_t0, W["in"], d))
    if kv is not None:  # the fold: the in-order fp32 sum of an image's slabs rounded once -- exact
        assert R.same_bits(o.dkv, S.kv_fold(kv[0].reshape(-1, kv[2], 2 * c), kv[1])), "kv fold"


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("c,rows,tile", [(64, 64, 32), (64, 16384, 64), (128, 64, 32)])
def test_head_bwd(O, c, rows, tile, fold):
    """Catches: d_n1 unrounded; a partial row of the wrong tile; a slab added out of order or a tile's
    slab skipped by the fold; the fold reading another image's slabs."""
    plan = S.StPlan.head_bwd(c, rows, part_rows=rows // tile + 2)
    expect(plan, tile=tile)
    g = _gen(c + rows)
    inp = Inputs()
    W = weights(g, c)
    d_qkv = inp.rows(rnd(g, rows, 3 * c, scale=0.1, dtype=BF16))
    d_t1, t0 = inp.rows(rnd(g, rows, c, scale=0.1, dtype=BF16)), inp.rows(rnd(g, rows, c, dtype=BF16))
    s1 = inp.keep(S.ln_stats(t0, LN_EPS, F32).contiguous())
    kv = None
    if fold:  # 3 images of 4 tiles and 20 keys
        kv = (inp.keep(rnd(g, 3 * 4 * 20, 2 * c)), 4, 20, 3)
    o, _ = run_head_bwd(O, W, transposed(W), inp, d_qkv, d_t1, t0, s1, rows, c, plan, kv)
    check_head_bwd(W, d_qkv, d_t1, t0, s1, o, plan, f"head-bwd c{c} r{rows} fold{int(fold)}", kv)
    inp.unchanged()


# ====================================================================== chained
@pytest.mark.parametrize("c", [64, 128, 256])
def test_chained(O, c):
    """Forward head, library self-attention, forward tail, backward tail, self-attention backward,
    backward head, each on the previous kernel's own outputs and each checked stage-locally: the saved
    layouts the backward reads (s2, s3 [rows][2]; lse2 [B * 8][tokens]; f [rows][8c] dense) are the ones
    the forward writes.  c = 256 has no fused backward: the forward chain (self statistics) only."""
    tokens, B, nctx = (64, 2, 20) if c < 256 else (16, 2, 20)
    rows, dh = B * tokens, c // 8
    train = c < 256
    h = HeadIn(c, tokens, B, seed=40 + c)
    form = "producer" if train else "self"
    hd = run_head_fwd(O, h, form, train)
    check_head_fwd(h, hd, f"chain{c} head", form, train)
    t = TailIn(c, tokens, B, nctx, seed=41 + c)
    t.W, t.x, t.t0 = h.W, h.x, hd.t0
    q, k, v = (hd.qkv[:, i * c:(i + 1) * c] for i in range(3))
    o1, lse1 = Guard(rows, c, BF16, strided=True), nan_guard(B * 8, tokens)
    O.attention_fwd(q, k, v, o1.view, lse1.view, B, 8, tokens, tokens, dh)
    t.o1 = o1.view
    plan = S.StPlan.tail_fwd(c, rows, tokens, nctx)
    expect(plan, tile=16)
    tl, _ = run_tail_fwd(O, t, train, False, False)
    if not train:
        tl2, _ = run_tail_fwd(O, t, True, False, False)
        check_tail_fwd(t, tl2, f"chain{c} tail", spl=plan.spl)
        assert R.same_bits(tl.out, tl2.out)
        return
    check_tail_fwd(t, tl, f"chain{c} tail", spl=plan.spl)
    bplan = S.StPlan.tail_bwd(c, rows, tokens, nctx, part_rows=rows // (64 if c == 64 else 32) + 3)
    expect(bplan, tile=64 if c == 64 else 32, mf=True, tpi=1 if c == 64 else 2)
    dy = t.inp.rows(rnd(_gen(50 + c), rows, c, scale=0.1, dtype=BF16))
    sv = NS(**{k: getattr(tl, k) for k in ("f", "t2", "t1", "q2", "o2", "s3", "s2", "lse2")})
    wt = transposed(t.W)
    tb, _ = run_tail_bwd(O, t, sv, dy, wt, bplan)
    check_tail_bwd(t, sv, dy, tb, bplan, f"chain{c} tail-bwd")
    d_qkv = Guard(rows, 3 * c, BF16, strided=True)
    dq, dk, dv = (d_qkv.view[:, i * c:(i + 1) * c] for i in range(3))
    O.attention_bwd(q, k, v, o1.view, lse1.view, tb.d_o1, dq, dk, dv, B, 8, tokens, tokens, dh)
    torch.cuda.synchronize()
    d_qkv.check()
    hplan = S.StPlan.head_bwd(c, rows, part_rows=rows // 32 + 2)
    expect(hplan, tile=32)
    kv = (tb.kv_part, bplan.tpi, nctx, B) if bplan.tpi > 1 else None
    hb, _ = run_head_bwd(O, t.W, wt, t.inp, d_qkv.view, tb.d_t1, hd.t0, hd.s1, rows, c, hplan, kv)
    check_head_bwd(t.W, d_qkv.view, tb.d_t1, hd.t0, hd.s1, hb, hplan, f"chain{c} head-bwd", kv)
    h.inp.unchanged()
    t.inp.unchanged()
