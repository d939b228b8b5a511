"""Per-element tests of the concept encoder's kernels on the MI355X: the training BatchNorm of
csrc/bn.hip (statistics and backward) and the warp MLPs and linear head of csrc/encoder.hip, each
against its fp64 restatement (tests/encoder_restate.py) on every dispatch path, by the method of
test_gpu_elementwise.py / test_gpu_st.py:
  * inputs are seeded on the host; every output is a view inside a sentinel- or NaN-filled Guard
    with a padded leading dimension, and every byte outside the view must be unchanged;
  * the inputs' buffers must be unchanged;
  * every launch runs twice from the same initial values and the two must agree bitwise (all three
    families add in a fixed order);
  * no tolerance is a constant chosen in advance: bf16 outputs follow the bf16 rule, fp32 outputs
    the fp32 rule, with floor = 4 x |fp32 evaluation - fp64| of the restatement on the case's own
    inputs, plus bounds derived from the kernels' serial summation order (encoder_restate's
    `*_slack`; the derivations are written there and next to their use below).

Kernel branch -> test
  bn_bwd_reduce_kernel<true>  (fp32 x) / <false> (bf16 x), relu 0 / 1,
    contiguous and ldx / lddy = c + 24 ................................. test_bn_bwd (every case)
    one pixel, pixel lanes with no row (rows 1) ........................ test_bn_bwd[1-8], [1-256]
    one workgroup, partly empty lanes (rows 50) ........................ test_bn_bwd[50-*]
    two workgroups, per = 129, the second short (rows 257) ............. test_bn_bwd[257-*]
    17 workgroups, last row alone in its 8-row unroll (rows 4099) ...... test_bn_bwd[4099-*]
    the 128-workgroup cap, per = 259, last range 132 rows .............. test_bn_bwd[33025-*]
    mask `<= 0` at z == 0 exactly (first / last row, channel 0 / c-1) .. test_bn_bwd (planted zeros)
    last row's last 8-channel vector (dy = 4 planted) .................. test_bn_bwd (planted tail)
    dgamma / dbeta += onto non-zero values, coef slot, counter reset ... test_bn_bwd
  bn_bwd_apply_kernel<true> / <false>: lddx = c + 24, c0 / c1 slots .... test_bn_bwd (every case)
    grid-stride second pass (33025 x 32 vectors > 4096 x 256) .......... test_bn_bwd[33025-256]
  bn_stats_kernel<true> / <false>: mean, rstd, running_mean / _var ..... test_bn_stats (same shapes)
  bn_bwd on the forward's own mean / rstd (as cond.py chains them) ..... test_bn_chained[8..256]
  bn_check / encdiff_batchnorm_bwd refusals ............................ test_bn_refusals
  encdiff_batchnorm_partials_floats .................................... test_bn_bwd, test_bn_stats
  warp_fwd_kernel: batch < one chunk (nr < 8), batch 1 ................. test_warp[1-1-16-0], [7-3-16-0]
    chunk edge 8 | 9, unit_stride > block (gap untouched) .............. test_warp[8-2-16-8], [9-2-16-8]
    production block with a 2-row tail ................................. test_warp[50-20-16-0]
    context_dim < 16: `e < nr * D` store guard, W3 / b3 offsets ........ test_warp[13-3-5-0], [13-3-1-4]
    ldu / ldo wider than the data ...................................... test_warp (every case)
  warp_bwd_kernel: `m < D` guards, `e < D * H2` partial store guard .... test_warp[13-3-5-0], [13-3-1-4]
    tail chunk's du (`tid < nr`), rows >= nr zeroed in dout / dz ....... test_warp[7-..], [9-..], [50-..]
    h1 pre-activation exactly 0 (ELU' from the output = 1) ............. test_warp (planted w1 = b1 = 0)
    lddo / lddu wider than the data .................................... test_warp (every case)
  warp_grad_reduce_kernel: chunks 1 / 2 / 7, += onto random grads,
    gaps between and after units bitwise unchanged ..................... test_warp
  warp entry points: ld narrower than the data refused (added here) .... test_warp_refusals
  head_fwd_kernel: units % 4 != 0 (`j >= units` waves), K % 64 tails,
    K = 384 not a multiple of 256, ldr = d + 8, ldu = units + 8 ........ test_head (every case)
  head_bwd_kernel<20>: units 7 (padded du, clamped W row), 20 .......... test_head[1-16-7], [5-24-20]
    d = 24: half-masked channel chunk (`kv`, `c2 >= d`) ................ test_head[5-24-20]
    batch < 16: empty image groups; batch 1 ............................ test_head[1-16-7], [5-..], [9-..]
  head_bwd_kernel<40>: units 33 (padded), 40 ........................... test_head[17-128-33], [257-16-40]
    staging boundary at batch 257 (group 15 spans both chunks) ......... test_head[257-16-40]
  head_bwd_kernel<64>: units 41 (padded), 64; 64 KB dynamic LDS ........ test_head[9-32-41], [9-32-64]
    <64> across the staging boundary ................................... test_head[300-16-64]
  head_bwd: dW / db += onto random values, lddr = d + 24, lddu + 8 ..... test_head (every case)
  head entry points: units 0 / 65, lddr < d; ldr < d and lddu < units
    in the backward (added here) ....................................... test_head_refusals

Found while writing these tests
  * 33025 x 128 is 528,400 8-channel vectors, under the apply kernels' 4096 x 256 grid cap: their
    second grid-stride pass needs c = 256 at that row count (1,056,800 vectors), so the case
    [33025-256] runs beside [33025-8] and [33025-128].
  * encdiff_encoder_head_bwd accepted ldr < d and lddu < units, and the warp entry points ldu / lddu
    < units and ldo / lddo < units * context_dim (they index with them): fixed here, ENCDIFF_ERR_ARG.
  * head_bwd_kernel<64> (units 41..64), launched here for the first time: the runtime accepts its
    64 KB dynamic LDS request as it is (no hipFuncSetAttribute needed) and dr / dW / db are within
    their bounds at units 41 and 64, below and across the du staging boundary.  Nothing to fix.
  * No kernel bug was found: the fp32-x backward, the strided forms and the `+=` all hold.

Measured on the MI355X (printed by the run: largest floor / largest |out - ref| / largest
fraction of the bound used, over every case of the output)
  output         floor     |out-ref|  bound used
  bn_dx          1.95e-06  7.81e-03   0.498   (bf16 rule; half a bf16 ulp of 2^-7 |ref| is 0.5)
  bn_dgamma      -         1.06e-04   0.096   (chain bound, no floor)
  bn_dbeta       -         3.15e-05   0.043
  bn_mean        -         1.97e-07   0.070
  bn_rstd        -         1.16e-07   0.221
  bn_rmean       -         2.75e-07   0.480
  bn_rvar        -         2.36e-07   0.180
  one row (rstd = eps^-1/2 ~ 316 scales dx by ~1e8; recorded apart): dx floor 6.9e+02, error
    3.3e+05, 0.359 of the bound; dgamma 0.148; dbeta 0.644 (the bound there is little more than the
    rounding of `prior + term`); mean exact; rstd 0.220; running_mean 0.693; running_var 0.376
  warp_out       1.37e-05  3.43e-06   0.0049
  warp_du        1.05e-04  4.25e-05   0.0008
  warp_dW1       5.40e-05  1.35e-05   0.0036
  warp_db1       3.46e-05  1.68e-05   0.0041
  warp_dW2       3.16e-05  5.87e-06   0.064
  warp_db2       1.25e-05  2.28e-06   0.030
  warp_dW3       2.83e-04  5.76e-05   0.017
  warp_db3       2.44e-05  4.17e-06   0.088
  head_u         1.69e-05  1.10e-06   0.032
  head_dr        2.01e-06  3.90e-03   0.999   (bf16 store: a correctly rounded value uses the half ulp)
  head_dW        1.76e-04  1.30e-05   0.105
  head_db        2.14e-05  9.00e-06   0.099
The outputs behind several stacked contractions use the least of their bound: n 2^-24 sum |a b| is a
worst case per contraction (a correct kernel's rounding errors grow like sqrt(n), not n) and the
worst cases multiply along the path.  61 % of du's bound is the 64-term z2 contraction's bound carried
through |dh2| |W2| |W1|; its median is 6e-3 at |du| ~ 3, where one dropped product of du's own 64-term
sum is ~0.4, tens of times the bound.  A dropped term, row or chunk is what these bounds must see,
and do (the dout = 64 and dy = 4 plants; each of the mutations listed in the change description
fails here).
"""
import ctypes
import os

import pytest
import torch

import elementwise_restate as R
import encoder_restate as E
from test_gpu_elementwise import BF16, F32, F64, Guard, _gen, assert_bf16_rule, dev, place, rnd
from test_gpu_st import STATS, Inputs, bound, twice

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -24
EPS32 = torch.tensor(1e-5, dtype=F32).item()   # EncdiffBatchNormArgs.eps / .momentum are floats
MOM32 = torch.tensor(0.1, dtype=F32).item()


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert "ENCDIFF_BN_MAXBLK" not in os.environ, \
        "ENCDIFF_BN_MAXBLK is set: these tests pin the workgroup ranges of bn.hip's default cap (128)"
    import encdiff_amd._lib as lib
    yield lib
    print("\noutput: largest floor / largest |out - ref| / largest fraction of the bound used")
    for k in sorted(k for k in STATS if k.startswith("enc:")):
        print(f"  {k:18s} {STATS[k][0]:.2e} {STATS[k][1]:.2e} {STATS[k][2]:.4f}")


@pytest.fixture(scope="module")
def O(L):
    from encdiff_amd import ops
    return ops


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _record(what, floor, err, used):
    st = STATS.setdefault(what.split()[-1], [0.0, 0.0, 0.0])
    st[0], st[1], st[2] = max(st[0], floor), max(st[1], err), max(st[2], used)


def within(what, out, ref64, tol):
    """|out - ref64| <= tol per element (tol: a derived bound, no floor), recorded like bound()"""
    assert out.shape == ref64.shape == tol.shape, (what, out.shape, ref64.shape, tol.shape)
    assert not torch.isnan(out).any(), f"{what}: NaN (unwritten or poisoned) in the output"
    err = (out.double() - ref64).abs()
    used = (err / tol.clamp_min(1e-300)).max().item()
    _record(what, 0.0, err.max().item(), used)
    print(f"{what}: max|out-ref| {err.max().item():.3e} bound used {used:.4f}")
    i = int((err - tol).argmax())
    assert (err <= tol).all(), (f"{what}: element {i} = {out.flatten()[i].item()!r} vs {ref64.flatten()[i].item()!r} "
                                f"exceeds the bound {tol.flatten()[i].item():.3e}")


def bf16_rule(what, out, ref64, t32):
    """the project's bf16 rule (2^-7 |ref| + floor), recorded"""
    assert_bf16_rule(out, ref64, t32, what)
    floor = R.floor_of(t32, ref64)
    err = (out.double() - ref64).abs()
    _record(what, floor, err.max().item(), (err / (2.0 ** -7 * ref64.abs() + floor).clamp_min(1e-300)).max().item())


def nan_out(rows, cols, dtype=F32, pad=64):
    """an output every element of which the kernel must write: NaN inside and around, ld = cols + 8"""
    return Guard(rows, cols, dtype, ld=cols + 8, left=0, fill=NAN, pad=pad,
                 init=torch.full((rows, cols), NAN, dtype=dtype, device=dev))


def keep_placed(inp, x, strided):
    """place() + the underlying buffer registered with the Inputs (unchanged() covers the padding too)"""
    v = place(x, strided)
    inp.keep(v._base if v._base is not None else v)
    return v


# ====================================================================== 1. BatchNorm
BN_SHAPES = [(1, 8), (1, 256), (50, 8), (50, 32), (50, 128), (50, 256), (257, 8), (257, 128),
             (4099, 8), (4099, 32), (4099, 128), (4099, 256), (33025, 8), (33025, 128), (33025, 256)]


def _partials(L, rows, c):
    n = L.lib.encdiff_batchnorm_partials_floats(rows, c)
    assert n == min((rows + 255) // 256, 128) * 2 * c + 2 * c
    return Guard(1, n, F32)


def _bn_args(L, rows, c, relu, x, gamma, beta, mean, rstd, part, cnt, **kw):
    return L.BatchNormArgs(rows=rows, c=c, eps=1e-5, momentum=0.1, relu=int(relu), x_f32=int(x.dtype == F32),
                           x=x.data_ptr(), ldx=x.stride(0), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                           mean=mean.data_ptr(), rstd=rstd.data_ptr(), partials=part.data_ptr(),
                           counter=cnt.data_ptr(), **kw)


def _z64(x, mean, rstd, gamma, beta):
    return (x.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()


def _bn_bwd_inputs(rows, c, xdt, seed):
    """Host-seeded inputs of one backward case (all on the host; the caller moves them).
    mean / rstd are the test's own: the fp64 batch statistics of x rounded to fp32 (of the first draw:
    the backward takes the caller's statistics as they are, and so does the restatement).
      * the ReLU mask is unambiguous: every element with |z| < 1e-3 (z in fp64) is redrawn until none
        remains -- asserted below, nothing is excluded from the comparison;
      * exact zeros: channels 0 and c - 1 have beta = 0 and a bf16-representable mean, and x of the
        first and last row there IS the mean, so z == 0 in any arithmetic and torch's relu' masks it;
      * dy = 4 in the last row's last 8-channel vector, whose x sits at xh ~ 3 (passes the ReLU)."""
    g = _gen(seed)
    x = (torch.randn(rows, c, generator=g) * 2 + 0.5).to(xdt)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.2
    beta[0] = beta[c - 1] = 0.0
    dy = torch.randn(rows, c, generator=g).to(BF16)
    x64 = x.double()
    mean = x64.mean(0).float()
    rstd = (1.0 / torch.sqrt(((x64 - x64.mean(0)) ** 2).mean(0) + EPS32)).float()
    for ch in (0, c - 1):
        mean[ch] = mean[ch].to(BF16).float()
    # xh >= 3 whatever the format and rstd (one row: rstd = eps^-1/2, so 3 / rstd is under a bf16 ulp of x)
    x[rows - 1, c - 8:] = (mean[c - 8:] + 3.0 / rstd[c - 8:] + mean[c - 8:].abs() * 2.0 ** -6).to(xdt)
    while True:
        bad = _z64(x, mean, rstd, gamma, beta).abs() < 1e-3
        if not bad.any():
            break
        x[bad] = (torch.randn(int(bad.sum()), generator=g) * 2 + 0.5).to(xdt)
    planted = torch.zeros(rows, c, dtype=torch.bool)
    for ch in (0, c - 1):
        for r in (0, rows - 1):
            x[r, ch] = mean[ch].to(xdt)
            planted[r, ch] = True
    dy[rows - 1, c - 8:] = 4.0
    z = _z64(x, mean, rstd, gamma, beta)
    assert (z[planted] == 0).all() and (z[~planted].abs() >= 1e-3).all()
    assert (z[rows - 1, max(c - 8, 1):c - 1] > 1e-3).all()  # the planted dy = 4 passes the ReLU
    return x, dy, mean, rstd, gamma, beta


def _bn_bwd_check(L, what, rows, c, relu, x, dy, mean, rstd, gamma, beta, strided, seed, planted_tail=True):
    """One backward form: launch twice from the same random dgamma / dbeta, Guards, inputs unchanged,
    counter 0, dx by the bf16 rule, dgamma / dbeta by the chain bound."""
    g = _gen(seed)
    inp = Inputs()
    xv, dyv = keep_placed(inp, x, strided), keep_placed(inp, dy, strided)
    for t in (mean, rstd, gamma, beta):
        inp.keep(t)
    dg0, db0 = rnd(g, 1, c, scale=3.0), rnd(g, 1, c, scale=3.0)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)

    def run():
        o = dict(dx=Guard(rows, c, BF16, strided=strided), dgamma=Guard(1, c, F32, init=dg0),
                 dbeta=Guard(1, c, F32, init=db0), partials=_partials(L, rows, c))
        a = _bn_args(L, rows, c, relu, xv, gamma, beta, mean, rstd, o["partials"].view, cnt,
                     dy=dyv.data_ptr(), lddy=dyv.stride(0), dx=o["dx"].view.data_ptr(), lddx=o["dx"].view.stride(0),
                     dgamma=o["dgamma"].view.data_ptr(), dbeta=o["dbeta"].view.data_ptr())
        L.check(L.lib.encdiff_batchnorm_bwd(ctypes.byref(a), _stream()), what)
        torch.cuda.synchronize()
        assert int(cnt.item()) == 0, "the arrival counter was not reset"
        for k in o:
            o[k].check()
        return o
    o, _ = twice(run)
    inp.unchanged()
    dx64, sg64, sgx64 = E.batchnorm_bwd(xv, dyv, mean, rstd, gamma, beta, relu, F64)
    dx32 = E.batchnorm_bwd(xv, dyv, mean, rstd, gamma, beta, relu, F32)[0]
    one = "_1row" if rows == 1 else ""  # one row: rstd = eps^-1/2 ~ 316 scales every figure; recorded apart
    bf16_rule(f"{what} enc:bn_dx{one}", o.dx, dx64, dx32)
    # dgamma / dbeta: the kernel adds a channel's terms serially in fp32 (torch's blocked fp32 sum is
    # no yardstick): a term passes at most depth = ceil(per / lanes) + lanes adds (its thread's rows,
    # then the LDS sum over the pixel lanes), each rounding a partial sum of magnitude <= sum |term|
    # by 2^-24; + 2 for the term's own product and the fp32 store of the fp64 fold;
    # + 2^-24 |prior + ref| for the `+=` into the gradient.
    xh = (xv.double() - mean.double()) * rstd.double()
    gm = dyv.double() * ((xh * gamma.double() + beta.double() > 0) if relu else 1.0)
    for name, terms, ref, prior, got in (("dbeta", gm, sg64, db0, o.dbeta), ("dgamma", gm * xh, sgx64, dg0, o.dgamma)):
        want = prior[0].double() + ref
        tol = E.bn_sum_slack(terms, rows, c) + U * want.abs()
        if planted_tail:  # a bound over one row's contribution proves nothing
            live = slice(max(c - 8, 1), c - 1)  # channels 0 and c - 1 hold the planted zeros
            assert (tol[live] < terms[rows - 1, live].abs()).all() and (terms[rows - 1, live].abs() >= 4.0).all()
        within(f"{what} enc:bn_{name}{one}", got[0], want, tol)


@pytest.mark.parametrize("rows,c", BN_SHAPES, ids=lambda v: str(v))
def test_bn_bwd(L, rows, c):
    """encdiff_batchnorm_bwd with fp32 and bf16 x, relu 0 / 1, contiguous and as column slices
    (ld = c + 24), dgamma / dbeta starting random, on the test's own mean / rstd.  Catches: the row
    loop ending one row early (dy = 4 planted in the last row), the last 8-channel vector dropped,
    fp32 x read with the bf16 stride, lddy / lddx taken for c, the mask `<` instead of `<=` at the
    planted z == 0, mean(g) and mean(g xh) read from each other's slot, `=` instead of `+=`, a
    counter left at the grid size, a second apply pass lost at [33025-256]."""
    for xdt in (F32, BF16):
        h = _bn_bwd_inputs(rows, c, xdt, seed=7000 + rows + c + (xdt == BF16))
        x, dy, mean, rstd, gamma, beta = (t.to(dev) for t in h)
        for relu in (0, 1):
            for strided in (False, True):
                what = f"bn_bwd {rows}x{c} x={'f32' if xdt == F32 else 'bf16'} relu={relu} strided={int(strided)}"
                _bn_bwd_check(L, what, rows, c, relu, x, dy, mean, rstd, gamma, beta, strided, seed=rows + c + relu)


def _bn_fwd(L, what, rows, c, relu, xv, gamma, beta, rm0, rv0):
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)

    def run():
        o = dict(y=Guard(rows, c, BF16, strided=True), mean=Guard(1, c, F32, fill=NAN), rstd=Guard(1, c, F32, fill=NAN),
                 rm=Guard(1, c, F32, init=rm0), rv=Guard(1, c, F32, init=rv0), partials=_partials(L, rows, c))
        a = _bn_args(L, rows, c, relu, xv, gamma, beta, o["mean"].view, o["rstd"].view, o["partials"].view, cnt,
                     y=o["y"].view.data_ptr(), ldy=o["y"].view.stride(0), running_mean=o["rm"].view.data_ptr(),
                     running_var=o["rv"].view.data_ptr())
        L.check(L.lib.encdiff_batchnorm_fwd(ctypes.byref(a), _stream()), what)
        torch.cuda.synchronize()
        assert int(cnt.item()) == 0, "the arrival counter was not reset"
        for k in o:
            o[k].check()
        return o
    return twice(run)[0]


@pytest.mark.parametrize("rows,c", BN_SHAPES, ids=lambda v: str(v))
def test_bn_stats(L, rows, c):
    """mean, rstd, running_mean, running_var of encdiff_batchnorm_fwd per channel, fp32 and bf16 x,
    contiguous and strided, running statistics starting at random values.  Bounds:
    encoder_restate.batchnorm_stats_slack (the chain bound on sum x and sum x^2 carried to each
    output + the fp32 rounding of the stored value).  Catches: the biased variance in running_var or
    the unbiased one under rstd, n - 1 = 0 at one row, momentum applied to the prior, a dropped row
    or lane (mean moves by x / n, far over the bound), running_* overwritten instead of blended."""
    g = _gen(8000 + rows + c)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), rnd(g, c, scale=0.2)
    rm0, rv0 = rnd(g, 1, c), (torch.rand(1, c, generator=g) + 0.5).to(dev)
    x32 = rnd(g, rows, c, scale=2.0) + 0.5
    for xdt in (F32, BF16):
        for strided in (False, True):
            inp = Inputs()
            xv = keep_placed(inp, x32.to(xdt), strided)
            what = f"bn_stats {rows}x{c} x={'f32' if xdt == F32 else 'bf16'} strided={int(strided)}"
            o = _bn_fwd(L, what, rows, c, 0, xv, gamma, beta, rm0, rv0)
            inp.unchanged()
            ref = E.batchnorm_stats(xv, EPS32, MOM32, rm0[0], rv0[0], F64)
            tol = E.batchnorm_stats_slack(xv, EPS32, MOM32, rm0[0], rv0[0])
            for name, got, r, t in zip(("mean", "rstd", "rmean", "rvar"), (o.mean, o.rstd, o.rm, o.rv), ref, tol):
                within(f"{what} enc:bn_{name}{'_1row' if rows == 1 else ''}", got[0], r, t)


@pytest.mark.parametrize("c", [8, 32, 128, 256])
def test_bn_chained(L, c):
    """As cond.py chains them: encdiff_batchnorm_fwd on fp32 x (ReLU), then encdiff_batchnorm_bwd on
    the mean / rstd that launch wrote, 4099 rows, strided.  The mask stays unambiguous: elements with
    |z| < 2e-3 under the fp64 batch statistics are redrawn (the statistics recomputed) until none
    remains, and |z| >= 1e-3 is asserted on the kernel's own statistics before the backward."""
    rows = 4099
    g = _gen(9000 + c)
    x = torch.randn(rows, c, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    while True:
        x64 = x.double()
        m64 = x64.mean(0)
        r64 = 1.0 / torch.sqrt(((x64 - m64) ** 2).mean(0) + EPS32)
        bad = _z64(x, m64, r64, gamma, beta).abs() < 2e-3
        if not bad.any():
            break
        x[bad] = torch.randn(int(bad.sum()), generator=g) * 2 + 0.5
    dy = torch.randn(rows, c, generator=g).to(BF16)
    dy[rows - 1, c - 8:] = 4.0
    x, gamma, beta, dy = (t.to(dev) for t in (x, gamma, beta, dy))
    rm0, rv0 = rnd(g, 1, c), (torch.rand(1, c, generator=g) + 0.5).to(dev)
    xv = place(x, True)
    o = _bn_fwd(L, f"bn_chained fwd c={c}", rows, c, 1, xv, gamma, beta, rm0, rv0)
    mean, rstd = o.mean[0].clone(), o.rstd[0].clone()
    assert (_z64(x, mean, rstd, gamma, beta).abs() >= 1e-3).all()
    _bn_bwd_check(L, f"bn_chained c={c}", rows, c, 1, x, dy, mean, rstd, gamma, beta, True, seed=c, planted_tail=False)


def test_bn_refusals(L):
    """Refused before any launch, by error code: c = 24 (8-channel vectors do not tile 256 threads)
    and c = 512 (the fold's limit); lddy / lddx not a multiple of 8; dgamma NULL; fp32 x misaligned
    by 4 bytes; mean misaligned.  Nothing is written and the counter stays 0."""
    rows = 16
    g = _gen(1)

    def attempt(c, xdt=BF16, x_off=0, mean_off=0, lddy=None, lddx=None, no_dgamma=False):
        x = rnd(g, rows * c + 8, dtype=xdt)[x_off:x_off + rows * c].view(rows, c)
        dy = rnd(g, rows, c, dtype=BF16)
        mean = torch.zeros(c + 8, device=dev)[mean_off:mean_off + c]
        rstd, gamma, beta = torch.ones(c, device=dev), torch.ones(c, device=dev), torch.zeros(c, device=dev)
        dx, dg, db = Guard(rows, c, BF16), Guard(1, c, F32), Guard(1, c, F32)
        part, cnt = Guard(1, 4 * c + 2 * c, F32), torch.zeros(1, device=dev, dtype=torch.int32)
        a = _bn_args(L, rows, c, 1, x, gamma, beta, mean, rstd, part.view, cnt, dy=dy.data_ptr(),
                     lddy=c if lddy is None else lddy, dx=dx.view.data_ptr(), lddx=c if lddx is None else lddx,
                     dgamma=None if no_dgamma else dg.view.data_ptr(), dbeta=db.view.data_ptr())
        rc = L.lib.encdiff_batchnorm_bwd(ctypes.byref(a), _stream())
        torch.cuda.synchronize()
        if rc:
            for t in (dx, dg, db, part):
                assert R.same_bits(t.buf, t.before)
        assert int(cnt.item()) == 0
        return rc
    assert attempt(16) == 0  # the same call, well formed, is accepted
    assert attempt(24) == -2 and attempt(512) == -2                     # ENCDIFF_ERR_SHAPE
    assert attempt(16, lddy=20) == -1 and attempt(16, lddx=20) == -1    # ENCDIFF_ERR_ARG
    assert attempt(16, no_dgamma=True) == -1
    assert attempt(16, xdt=F32, x_off=1) == -1
    assert attempt(16, mean_off=1) == -1


# ====================================================================== 2. warp MLPs
WARP_CASES = [(1, 1, 16, 0), (7, 3, 16, 0), (8, 2, 16, 8), (9, 2, 16, 8), (50, 20, 16, 0), (13, 3, 5, 0), (13, 3, 1, 4)]
WARP_SEGS = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


def _warp_params(g, units, D, stride):
    """unit blocks at `stride`, NaN in the gaps (a read of a gap poisons the output); scales chosen so
    that both ELU branches occur in h1 and h2; one h1 pre-activation of unit 0 exactly 0"""
    npu = E.warp_n_per_unit(D)
    P = torch.full((units, stride), NAN)
    sc = torch.cat([torch.full((64,), 1.0), torch.full((64,), 0.5), torch.full((128 * 64,), 0.25), torch.full((128,), 0.3),
                    torch.full((D * 128,), 128 ** -0.5), torch.full((D,), 0.1)])
    P[:, :npu] = torch.randn(units, npu, generator=g) * sc
    P[0, 5] = 0.0        # w1[5]
    P[0, 64 + 5] = 0.0   # b1[5]
    return P.reshape(-1).to(dev)


@pytest.mark.parametrize("B,units,D,gap", WARP_CASES, ids=lambda v: str(v))
def test_warp(O, B, units, D, gap):
    """ops.encoder_warp_fwd / _bwd on raw tensors: u, out, dout, du are column views of buffers 8
    columns wider (NaN beyond), `grads` starts random with its gaps guarded.  All fp32: the fp32 rule
    + encoder_restate.warp_slack (the serial 64- and 128-term contractions, the chunk-ordered batch
    sums and expm1f, carried through |weights|).  One dout of 64 in the last row.  Catches: the tail
    chunk's du written for 8 rows or not at all, rows >= nr of a tail chunk leaking into the
    gradients, W3 / b3 taken at the D = 16 offsets, a gradient written into the unit gap, `=` for `+=`
    in the reduce, chunk partials of another unit, ELU' taken from the pre-activation."""
    npu, stride = E.warp_n_per_unit(D), E.warp_n_per_unit(D) + gap
    g = _gen(100 * B + 10 * units + D)
    inp = Inputs()
    params = inp.keep(_warp_params(g, units, D, stride))
    u = inp.rows(rnd(g, B, units))
    dout_h = torch.randn(B, units * D, generator=g)
    dout_h[B - 1, units * D - 1] = 64.0
    dout = inp.rows(dout_h.to(dev))
    grads0 = rnd(g, 1, units * stride)
    z1, _, z2, _ = E.warp_hidden(u, params, stride, units, D, F64)
    for z in (z1, z2):  # both ELU branches in the fp64 reference
        assert 0.2 <= (z < 0).double().mean().item() <= 0.8
    assert z1[0, :, 5].abs().max().item() == 0.0

    def run():
        # du's padding holds a whole stray chunk: 8 rows written for a 2-row tail land inside it
        o = dict(out=nan_out(B, units * D), du=nan_out(B, units, pad=64 + 8 * (units + 8)),
                 grads=Guard(1, units * stride, F32, init=grads0))
        O.encoder_warp_fwd(u, params, stride, units, D, o["out"].view)
        O.encoder_warp_bwd(u, params, stride, units, D, dout, o["du"].view, o["grads"].view[0])
        torch.cuda.synchronize()
        for k in o:
            o[k].check()
        return o
    o, _ = twice(run)
    inp.unchanged()
    what = f"warp B={B} units={units} D={D} gap={gap}"
    s_out, s_du, s_G = E.warp_slack(u, params, stride, units, D, dout)
    bound(what + " enc:warp_out", o.out, (E.warp_fwd(u, params, stride, units, D, F64),
                                         E.warp_fwd(u, params, stride, units, D, F32)), slack=s_out, store=False)
    du64, G64 = E.warp_bwd(u, params, stride, units, D, dout, F64)
    du32, G32 = E.warp_bwd(u, params, stride, units, D, dout, F32)
    bound(what + " enc:warp_du", o.du, (du64, du32), slack=s_du, store=False)
    got = o.grads[0].view(units, stride)
    assert R.same_bits(got[:, npu:], grads0[0].view(units, stride)[:, npu:]), "a gap of `grads` was written"
    w64 = (grads0[0].double() + G64).view(units, stride)
    w32 = (grads0[0] + G32).view(units, stride)
    sizes = [64, 64, 128 * 64, 128, D * 128, D]
    c0 = 0
    for name, n in zip(WARP_SEGS, sizes):
        sl = slice(c0, c0 + n)
        bound(f"{what} enc:warp_{name}", got[:, sl], (w64[:, sl], w32[:, sl]), slack=s_G.view(units, stride)[:, sl], store=False)
        c0 += n


def test_warp_refusals(L):
    """Leading dimensions narrower than the data are refused (ENCDIFF_ERR_ARG) before any launch:
    ldu / lddu < units, ldo / lddo < units * context_dim; context_dim 0 / 17 and a unit_stride below
    the parameter block keep their codes."""
    B, units, D = 4, 3, 16
    n = E.warp_n_per_unit(D)
    u, params = torch.zeros(B, units, device=dev), torch.zeros(units * n, device=dev)
    out, du = Guard(B, units * D, F32), Guard(B, units, F32)
    dout, grads = torch.zeros(B, units * D, device=dev), Guard(1, units * n, F32)
    part = Guard(1, L.lib.encdiff_encoder_warp_partials_floats(B, units, n), F32)

    def fwd(ldu=units, ldo=units * D, D_=D, stride=n):
        return L.lib.encdiff_encoder_warp_fwd(u.data_ptr(), ldu, B, units, params.data_ptr(), stride, D_,
                                              out.view.data_ptr(), ldo, _stream())

    def bwd(ldu=units, lddo=units * D, lddu=units, D_=D, stride=n):
        return L.lib.encdiff_encoder_warp_bwd(u.data_ptr(), ldu, B, units, params.data_ptr(), stride, D_, dout.data_ptr(),
                                              lddo, du.view.data_ptr(), lddu, grads.view.data_ptr(), part.view.data_ptr(),
                                              _stream())
    assert fwd(ldu=units - 1) == -1 and fwd(ldo=units * D - 1) == -1
    assert bwd(ldu=units - 1) == -1 and bwd(lddo=units * D - 1) == -1 and bwd(lddu=units - 1) == -1
    assert fwd(D_=0) == -3 and fwd(D_=17) == -3 and bwd(D_=17) == -3
    assert fwd(stride=n - 1) == -2 and bwd(stride=n - 1) == -2
    torch.cuda.synchronize()
    for t in (out, du, grads, part):
        assert R.same_bits(t.buf, t.before)


# ====================================================================== 3. linear head
HEAD_CASES = [(1, 16, 7), (5, 24, 20), (17, 128, 33), (257, 16, 40), (9, 32, 41), (9, 32, 64), (300, 16, 64)]


@pytest.mark.parametrize("B,d,units", HEAD_CASES, ids=lambda v: str(v))
def test_head(L, B, d, units):
    """encdiff_encoder_head_fwd / _bwd: r with ldr = d + 8, u and du with ld = units + 8 (NaN
    beyond), dr (bf16) in a strided Guard, dW / db starting random.  u, dW, db: the fp32 rule +
    encoder_restate.head_slack (the lane / wave, image-group and batch chains); dr: the same slack
    under the bf16 store.  Catches: the last channel chunk of d = 24 skipped or written past d, padded
    units (7, 33, 41) reading du or W beyond `units`, an image group's range wrong where groups are
    empty (B < 16) or span the staging boundary (B = 257, 300), W column c * 16 + p transposed,
    `=` for `+=`, <64>'s 64 KB LDS request refused or its partials overlapping."""
    K = d * 16
    g = _gen(B + d + units)
    inp = Inputs()
    r = inp.rows(rnd(g, B * 16, d))
    W = inp.keep(rnd(g, units, K, scale=0.05))
    bias = inp.keep(rnd(g, units))
    du = inp.rows(rnd(g, B, units))
    dW0, db0 = rnd(g, units, K), rnd(g, 1, units)
    what = f"head B={B} d={d} units={units}"

    def run():
        o = dict(u=nan_out(B, units), dr=Guard(B * 16, d, BF16, strided=True, fill=NAN),
                 dW=Guard(units, K, F32, init=dW0), db=Guard(1, units, F32, init=db0))
        L.check(L.lib.encdiff_encoder_head_fwd(r.data_ptr(), r.stride(0), B, d, W.data_ptr(), bias.data_ptr(), units,
                                               o["u"].view.data_ptr(), o["u"].view.stride(0), _stream()), what + " fwd")
        L.check(L.lib.encdiff_encoder_head_bwd(r.data_ptr(), r.stride(0), B, d, W.data_ptr(), units, du.data_ptr(),
                                               du.stride(0), o["dr"].view.data_ptr(), o["dr"].view.stride(0),
                                               o["dW"].view.data_ptr(), o["db"].view.data_ptr(), _stream()), what + " bwd")
        torch.cuda.synchronize()
        for k in o:
            o[k].check()
        return o
    o, _ = twice(run)
    inp.unchanged()
    s_u, s_dr, s_dW, s_db = E.head_slack(r, W, bias, du)
    bound(what + " enc:head_u", o.u, lambda dt: E.head_fwd(r, W, bias, dt), slack=s_u, store=False)
    b64, b32 = E.head_bwd(r, W, du, F64), E.head_bwd(r, W, du, F32)
    bound(what + " enc:head_dr", o.dr, (b64[0], b32[0]), slack=s_dr, store=True)
    bound(what + " enc:head_dW", o.dW, (dW0.double() + b64[1], dW0 + b32[1]), slack=s_dW, store=False)
    bound(what + " enc:head_db", o.db[0], (db0[0].double() + b64[2], db0[0] + b32[2]), slack=s_db, store=False)


def test_head_refusals(L):
    """units 65 and 0, lddr < d, and (added with these tests) ldr < d and lddu < units in the
    backward are refused with ENCDIFF_ERR_ARG before any launch; the forward refuses ldr < d and
    ldu < units."""
    B, d = 3, 16
    K = d * 16
    r, W, bias = torch.zeros(B * 16, d, device=dev), torch.zeros(65, K, device=dev), torch.zeros(65, device=dev)
    du = torch.zeros(B, 65, device=dev)
    u, dr, dW, db = Guard(B, 65, F32), Guard(B * 16, d, BF16), Guard(65, K, F32), Guard(1, 65, F32)

    def fwd(units=20, ldr=d, ldu=65):
        return L.lib.encdiff_encoder_head_fwd(r.data_ptr(), ldr, B, d, W.data_ptr(), bias.data_ptr(), units,
                                              u.view.data_ptr(), ldu, _stream())

    def bwd(units=20, ldr=d, lddu=65, lddr=d):
        return L.lib.encdiff_encoder_head_bwd(r.data_ptr(), ldr, B, d, W.data_ptr(), units, du.data_ptr(), lddu,
                                              dr.view.data_ptr(), lddr, dW.view.data_ptr(), db.view.data_ptr(), _stream())
    assert bwd(units=65) == -1 and bwd(units=0) == -1 and bwd(lddr=d - 1) == -1
    assert bwd(ldr=d - 1) == -1 and bwd(lddu=19) == -1
    assert fwd(units=0) == -1 and fwd(ldr=d - 1) == -1 and fwd(ldu=19) == -1
    torch.cuda.synchronize()
    for t in (u, dr, dW, db):
        assert R.same_bits(t.buf, t.before)
