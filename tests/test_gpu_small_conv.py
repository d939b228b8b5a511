"""Per-element tests of the 3-channel convolutions of csrc/elementwise.hip on the MI355X
(encdiff_small_conv_fwd / encdiff_small_conv_bwd) against tests/smallconv_restate.py in fp64.

Exact mode: activations and gradients are integers in [-8, 8], weights, biases in [-4, 4], prior
dW / db in [-64, 64].  The largest sum is 9 * 512 * 32 + 4 = 147,460 for an output (cin = 512)
and 576 * 64 + 64 = 36,928 for a weight gradient (one 24 x 24 image): every partial sum is
an integer below 2^24, exact in fp32 in any order, so fp32 outputs must equal the fp64 value cast to
fp32 bit for bit and bf16 outputs its round-to-nearest-even bf16 -- a wrong tap, channel, border,
lane fold or lap shows at the element, with no tolerance.
Rounded mode: seeded randn (bf16 where the kernel reads bf16, with the specials of `rnd`), compared
per element under the rules of tests/elementwise_restate.py with the floor measured at run time
(4 x the largest |torch fp32 evaluation - fp64| of the same restatement on the case's inputs).
Every output lies in a sentinel-filled `Guard`; check() proves nothing outside it changed.

Kernel branch -> test
  small_conv_out_fwd_lanes: vshift 0 (no shuffle) / 1 / 3 / 6, cout 3 / 1,
    1xN, Nx1, 1x1, h != w, strided x ................................. test_out_fwd_lanes
  small_conv_out_fwd_lanes: grid-stride second lap (270,400 lanes) ..... test_out_fwd_lanes_second_lap
  small_conv_out_fwd: cin 24 / 96 / 192, cout 3 / 1, strided x ......... test_out_fwd_pixel
  small_conv_out_fwd: grid-stride second lap (1,050,625 pixels) ........ test_out_fwd_pixel_second_lap
  small_conv_out_dgrad: cin 8 / 24 / 64 / 512, cout 3 / 1, strided dx .. test_out_dgrad
  small_conv_out_dgrad: grid-stride second lap ......................... test_out_dgrad_second_lap
  small_conv_in_fwd: cin 1 / 3 / 4, cout 8 / 64, strided y ............. test_in_fwd
  small_conv_in_fwd: grid-stride second lap (1,050,625 pixels) ......... test_in_fwd_second_lap
  small_conv_wgrad: both operand forms, batch 1 / 2 / 3 / 5 (odd: the
    two-image workgroup's tail), dbias present / NULL, accumulation onto
    prior values, 1728 weights (six full blocks + 192), LDS limit 24x24  test_wgrad
  small_conv_wgrad: 25 x 25 at cin 64 refused (LDS) .................... test_wgrad_refuses_over_lds
  all five kernels on randn inputs, (3,5,7) and (2,16,16) .............. test_rounded
  the launchers' argument refusals (no GPU needed) ..................... test_smallconv_restate.py
"""
import ctypes as C

import pytest
import torch

import elementwise_restate as R
import smallconv_restate as S
from test_gpu_elementwise import Guard, _gen, assert_bf16_rule, assert_f32_rule, place, rnd

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GEOMS = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 5, 7), (2, 16, 16)]


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    return ops


def _ints(g, lo, hi, *shape, dtype=F32):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(dev)


def _vals(g, exact, bound, *shape, dtype=F32, scale=1.0, specials=False):
    if exact:
        return _ints(g, -bound, bound, *shape, dtype=dtype)
    return rnd(g, *shape, scale=scale, dtype=dtype, specials=specials)


def _compare(out, ev, exact, what):
    """out against ev(F64): bitwise in exact mode, the project's per-element rule otherwise."""
    ref = ev(F64)
    if exact:
        want = ref.to(out.dtype)
        bad = (R.bits(out.contiguous()) != R.bits(want.contiguous())).flatten().nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} elements differ, first at flat index {int(bad[0])}: got "
                                  f"{out.flatten()[int(bad[0])].item()} want {want.flatten()[int(bad[0])].item()}")
    else:
        (assert_f32_rule if out.dtype == F32 else assert_bf16_rule)(out, ref, ev(F32), what)


# ====================================================================== output conv, forward
def _out_fwd(O, B, h, w, cin, cout, strided, exact, seed):
    g = _gen(seed)
    pix = B * h * w
    x = _vals(g, exact, 8, pix, cin, dtype=BF16, specials=True)
    wt = _vals(g, exact, 4, cout, cin, 3, 3, scale=(9 * cin) ** -0.5)
    b = _vals(g, exact, 4, cout)
    xv = place(x, strided)
    y = Guard(B * cout, h * w, F32)  # fp32 NCHW: contiguous by definition
    O.small_conv_out_fwd(xv, O.Geom(B, h, w), wt, b, y.view)
    torch.cuda.synchronize()
    y.check()
    _compare(y.view.reshape(B, cout, h, w),
             lambda dt: S.conv3x3(S.rows_to_nchw(x.to(dt), B, h, w), wt.to(dt), b.to(dt)), exact,
             f"out fwd ({B},{h},{w}) cin={cin} cout={cout} strided={int(strided)}")


@pytest.mark.parametrize("cin", [8, 16, 64, 512])
def test_out_fwd_lanes(O, cin):
    """The lane-group forward (cin / 8 a power of two): 1 lane per pixel (cin = 8, no shuffle), 2, 8
    and 64 (a whole wave per pixel), cout 3 and 1, every geometry, x contiguous and as a column slice
    (ld = cin + 24, first column 8).  Exact mode; the largest sum is 9 * 512 * 32 + 4 = 147,460.
    Catches: a tap with dy / dx exchanged (1xN against Nx1), h and w exchanged (5x7), the left / right
    border wrapping into the neighbouring row, the bottom row of image b reading image b + 1, a lane
    group folded over the wrong xor distance, cout = 1 writing channels 1 and 2 (the Guard), the row
    stride taken for cin."""
    for cout in (3, 1):
        for B, h, w in GEOMS:
            for strided in (False, True):
                _out_fwd(O, B, h, w, cin, cout, strided, True, seed=100 + cin + h * w + cout)


def test_out_fwd_lanes_second_lap(O):
    """cin = 512 at (1, 65, 65): 4225 pixels x 64 lanes = 270,400 lane-threads against the 1024
    workgroups x 256 of the capped grid -- one full lap and a ragged second one (8,256 lanes)."""
    _out_fwd(O, 1, 65, 65, 512, 3, True, True, seed=150)


@pytest.mark.parametrize("cin", [24, 96, 192])
def test_out_fwd_pixel(O, cin):
    """The thread-per-pixel forward (cin / 8 not a power of two), cout 3 and 1, every geometry,
    contiguous and strided x.  Exact mode (sums <= 9 * 192 * 32 + 4).  Catches the same index
    mistakes as the lane kernel's test, and the [co][tap][ci] weight reorder in LDS going wrong."""
    for cout in (3, 1):
        for B, h, w in GEOMS:
            for strided in (False, True):
                _out_fwd(O, B, h, w, cin, cout, strided, True, seed=200 + cin + h * w + cout)


def test_out_fwd_pixel_second_lap(O):
    """cin = 24 at (1, 1025, 1025): 1,050,625 pixels against 4096 workgroups x 256 threads, so the
    last 2,049 pixels belong to the stride loop's second lap.  The fp64 reference runs on the device."""
    _out_fwd(O, 1, 1025, 1025, 24, 3, True, True, seed=250)


# ====================================================================== output conv, input gradient
def _dgrad(O, B, h, w, cin, cout, strided, exact, seed):
    g = _gen(seed)
    pix = B * h * w
    dy = _vals(g, exact, 8, B, cout, h, w, specials=True)
    wt = _vals(g, exact, 4, cout, cin, 3, 3, scale=27 ** -0.5)
    x = torch.zeros(pix, cin, dtype=BF16, device=dev)  # not read without dweight
    dx = Guard(pix, cin, BF16, strided=strided)
    O.small_conv_out_bwd(x, O.Geom(B, h, w), wt, dy, dx.view, None, None)
    torch.cuda.synchronize()
    dx.check()
    _compare(dx.view, lambda dt: S.nchw_to_rows(S.conv3x3_dx(dy.to(dt), wt.to(dt))), exact,
             f"out dgrad ({B},{h},{w}) cin={cin} cout={cout} strided={int(strided)}")


@pytest.mark.parametrize("cin", [8, 24, 64, 512])
def test_out_dgrad(O, cin):
    """dx of the output conv: one thread per (pixel, 8 channels), cout 3 and 1, every geometry, dx
    contiguous and a strided Guard.  Exact mode: |dx| <= 27 * 32 = 864, rounded to bf16 (nearest
    even) as the fp64 value is.  Catches: the transposed tap offset taken with the forward's sign
    (1xN, Nx1, 5x7), cout = 1 reading dy channels 1 and 2 of the next image, a channel chunk written
    to the neighbouring pixel's row when lddx != cin, truncation instead of rounding."""
    for cout in (3, 1):
        for B, h, w in GEOMS:
            for strided in (False, True):
                _dgrad(O, B, h, w, cin, cout, strided, True, seed=300 + cin + h * w + cout)


def test_out_dgrad_second_lap(O):
    """cin = 512 at (1, 65, 65): 270,400 threads, a full lap of the capped grid and a ragged second."""
    _dgrad(O, 1, 65, 65, 512, 3, True, True, seed=350)


# ====================================================================== input conv, forward
def _in_fwd(O, B, h, w, cin, cout, strided, exact, seed):
    g = _gen(seed)
    pix = B * h * w
    x = _vals(g, exact, 8, B, cin, h, w, specials=True)
    wt = _vals(g, exact, 4, cout, cin, 3, 3, scale=(9 * cin) ** -0.5)
    b = _vals(g, exact, 4, cout)
    y = Guard(pix, cout, BF16, strided=strided)  # strided: ld = cout + 24, a multiple of 8
    O.small_conv_in_fwd(x, O.Geom(B, h, w), wt, b, y.view)
    torch.cuda.synchronize()
    y.check()
    _compare(y.view, lambda dt: S.nchw_to_rows(S.conv3x3(x.to(dt), wt.to(dt), b.to(dt))), exact,
             f"in fwd ({B},{h},{w}) cin={cin} cout={cout} strided={int(strided)}")


@pytest.mark.parametrize("cin,cout", [(1, 8), (3, 8), (4, 8), (1, 64), (3, 64), (4, 64)])
def test_in_fwd(O, cin, cout):
    """The input conv (fp32 NCHW -> bf16 rows), every geometry, y contiguous and strided.  Exact mode:
    |y| <= 36 * 32 + 4 = 1156, rounded to bf16.  Catches: the unused register taps of cin < 4 read
    from the next image, the channel stride h * w taken as w * w, the bias of channel c0 + j read at
    j, an 8-channel group written at the wrong column of a strided row."""
    for B, h, w in GEOMS:
        for strided in (False, True):
            _in_fwd(O, B, h, w, cin, cout, strided, True, seed=400 + cin + cout + h * w)


def test_in_fwd_second_lap(O):
    """cin = 3, cout = 8 at (1, 1025, 1025): 1,050,625 pixels, 2,049 of them in the second lap."""
    _in_fwd(O, 1, 1025, 1025, 3, 8, True, True, seed=450)


# ====================================================================== weight / bias gradient
def _wgrad(O, form, B, h, w, cin, cout, strided, with_bias, exact, seed):
    g = _gen(seed)
    pix = B * h * w
    geom = O.Geom(B, h, w)
    wt = torch.zeros(cout, cin, 3, 3, device=dev)  # shapes only: the weight gradient does not read it
    dw0 = _vals(g, exact, 64, cout, cin * 9)
    db0 = _vals(g, exact, 64, 1, cout)
    dw = Guard(cout, cin * 9, F32, init=dw0)
    db = Guard(1, cout, F32, init=db0) if with_bias else None
    dbv = db.view.view(-1) if with_bias else None
    if form == "in":  # x fp32 NCHW, dy bf16 rows
        x = _vals(g, exact, 8, B, cin, h, w, specials=True)
        dy = _vals(g, exact, 8, pix, cout, dtype=BF16)
        O.small_conv_in_wgrad(x, geom, wt, place(dy, strided), dw.view, dbv)
        nchw = lambda dt: (x.to(dt), S.rows_to_nchw(dy.to(dt), B, h, w))
    else:  # x bf16 rows, dy fp32 NCHW
        x = _vals(g, exact, 8, pix, cin, dtype=BF16, specials=True)
        dy = _vals(g, exact, 8, B, cout, h, w)
        O.small_conv_out_bwd(place(x, strided), geom, wt, dy, None, dw.view, dbv)
        nchw = lambda dt: (S.rows_to_nchw(x.to(dt), B, h, w), dy.to(dt))
    torch.cuda.synchronize()
    dw.check()
    what = f"wgrad {form} ({B},{h},{w}) cin={cin} cout={cout} strided={int(strided)} bias={int(with_bias)}"
    _compare(dw.view, lambda dt: dw0.to(dt) + S.conv3x3_dw(*nchw(dt)).reshape(cout, cin * 9), exact, what + " dW")
    if with_bias:
        db.check()
        _compare(db.view, lambda dt: db0.to(dt) + S.conv3x3_db(nchw(dt)[1]).view(1, cout), exact, what + " db")


@pytest.mark.parametrize("form", ["in", "out"])
def test_wgrad(O, form):
    """dW and db of either small conv, added onto non-zero prior values.  The in-conv form reads fp32
    NCHW x and bf16 rows dy, the out-conv form bf16 rows x and fp32 NCHW dy; the bf16 operand is
    contiguous and a column slice.  Batches 1 / 2 / 3 / 5 at 5 x 7: a workgroup takes two images, so
    odd batches leave a one-image tail.  cin = 64, cout = 3 (and 3 -> 64): 1728 weights, six full
    blocks of 256 and one of 192.  (1, 24, 24) at cin = 64 stages 67 x 576 floats = 154,368 B of the
    163,840 B of LDS.  Exact mode: |dW| <= 576 * 64 + 64.  The per-image-group partial sums are
    added with float atomics, whose order is not fixed: the integer sums here are exact in any order,
    so bitwise equality holds, but on rounded inputs with batch > 2 two runs may differ in the last
    bits -- run-to-run equality is deliberately not asserted there.
    Catches: an odd batch's last image dropped or read twice, a tap's valid range off by one at a
    border (1xN, Nx1, 1x1), dbias written when NULL or summed over the wrong channel, prior values
    overwritten, the last 192 weights skipped, x indexed with the row stride of dy."""
    shapes = [(3, 64), (1, 8), (4, 8)] if form == "in" else [(64, 3), (8, 1), (24, 3)]
    seed = 500 if form == "in" else 600
    for cin, cout in shapes:
        for B in (1, 2, 3, 5):
            for with_bias in (True, False):
                _wgrad(O, form, B, 5, 7, cin, cout, B % 2 == 1, with_bias, True, seed + B + cin)
        for B, h, w in GEOMS:
            for strided in (False, True):
                _wgrad(O, form, B, h, w, cin, cout, strided, True, True, seed + 50 + h * w + cin)
    cin, cout = shapes[0]
    _wgrad(O, form, 1, 24, 24, cin, cout, True, True, True, seed + 99)


def test_wgrad_refuses_over_lds(O):
    """(1, 25, 25) at cin = 64, cout = 3 needs 67 x 625 x 4 B = 167,500 B of LDS: ENCDIFF_ERR_SHAPE
    before any launch, dW untouched."""
    import encdiff_amd._lib as L
    x = torch.zeros(625, 64, dtype=BF16, device=dev)
    dy = torch.zeros(1, 3, 25, 25, device=dev)
    wt = torch.zeros(3, 64, 3, 3, device=dev)
    dw = Guard(3, 576, F32)
    a = L.SmallConvArgs(batch=1, h=25, w=25, cin=64, cout=3, x=x.data_ptr(), ldx=64, x_f32=0, weight=wt.data_ptr(),
                        dy=dy.data_ptr(), dy_f32=1, dweight=dw.view.data_ptr())
    assert L.lib.encdiff_small_conv_bwd(C.byref(a), None) == -2
    torch.cuda.synchronize()
    assert R.same_bits(dw.buf, dw.before)


# ====================================================================== rounded mode
@pytest.mark.parametrize("B,h,w", [(3, 5, 7), (2, 16, 16)], ids=str)
@pytest.mark.parametrize("kernel", ["out_fwd_lanes", "out_fwd_pixel", "out_dgrad", "in_fwd", "wgrad_in", "wgrad_out"])
def test_rounded(O, kernel, B, h, w):
    """Each kernel once on randn inputs (bf16 where it reads bf16; +-0, +-30, +-90 and values at
    bf16's smallest normal at both ends) at the UNet's cin = 64 (24 for the per-pixel forward, 3 -> 64
    for the input conv), per element: fp32 outputs within floor + 2^-22 |ref|, bf16 outputs within
    floor + 2^-7 |ref|, floor = 4 x max |torch fp32 - fp64| measured on the same inputs and printed.
    Measured on the MI355X, floor / worst |out - ref| at (3,5,7) and at (2,16,16):
      out_fwd_lanes   4.1e-6 / 8.5e-7    3.9e-6 / 7.3e-7
      out_fwd_pixel   1.0e-5 / 9.8e-6    1.8e-5 / 4.7e-6
      out_dgrad       2.9e-5 / 0.25      3.5e-5 / 0.22     (bf16: the rounding of |dx| up to ~60)
      in_fwd          5.0e-5 / 0.24      3.4e-5 / 0.18     (bf16)
      wgrad_in  dW    2.7e-4 / 9.1e-5    1.1e-3 / 3.5e-4   db  3.8e-6 / 9.5e-7    7.9e-6 / 2.0e-6
      wgrad_out dW    1.5e-4 / 5.0e-5    4.1e-4 / 2.2e-4   db  1.1e-5 / 1.7e-6    1.3e-5 / 1.3e-5
    The last db is the closest call: 512 terms summed in one sequential fp32 chain per channel,
    1.325e-5 against 1.269e-5 + 2^-22 |ref| (batch 2 is one workgroup: no atomics order in it)."""
    seed = 700 + h * w
    if kernel == "out_fwd_lanes":
        _out_fwd(O, B, h, w, 64, 3, True, False, seed)
    elif kernel == "out_fwd_pixel":
        _out_fwd(O, B, h, w, 24, 3, True, False, seed)
    elif kernel == "out_dgrad":
        _dgrad(O, B, h, w, 64, 3, True, False, seed)
    elif kernel == "in_fwd":
        _in_fwd(O, B, h, w, 3, 64, True, False, seed)
    elif kernel == "wgrad_in":
        _wgrad(O, "in", B, h, w, 3, 64, True, True, False, seed)
    else:
        _wgrad(O, "out", B, h, w, 64, 3, True, True, False, seed)
