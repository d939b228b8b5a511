"""CPU tests of tests/smallconv_restate.py (the reference of tests/test_gpu_small_conv.py) and of
the host-side refusals of encdiff_small_conv_fwd / encdiff_small_conv_bwd.

The restatement is held to torch.nn.functional.conv2d and its fp64 autograd on the geometries the
GPU tests use, bitwise on small integers (every partial sum is an integer below 2^24, exact in any
order).  Three deliberately wrong variants show that this exact comparison rejects the mistakes it
is there to catch.  The refusals need no GPU: every one returns before any launch, so the
pointers are plain numbers that are never dereferenced."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as Fn

import smallconv_restate as S
from elementwise_restate import same_bits

F64 = torch.float64
GEOMS = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 5, 7), (2, 16, 16)]


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _case(B, h, w, ci, co, seed):
    g = torch.Generator().manual_seed(seed)
    return (_ints(g, -8, 8, B, ci, h, w), _ints(g, -4, 4, co, ci, 3, 3), _ints(g, -4, 4, co),
            _ints(g, -8, 8, B, co, h, w))


@pytest.mark.parametrize("B,h,w", GEOMS)
@pytest.mark.parametrize("ci,co", [(3, 8), (1, 64), (8, 3), (24, 1), (64, 3)])
def test_restatement_matches_conv2d_and_autograd(B, h, w, ci, co):
    """Integers: |x|, |dy| <= 8, |w|, |b| <= 4, at most 9 * 64 * 32 + 4 per output and
    512 * 64 per weight gradient -- all sums exact in fp64 (and in fp32)."""
    x, wt, b, dy = _case(B, h, w, ci, co, seed=B * 100 + h * 10 + w + ci)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, wt, b))
    ref = Fn.conv2d(xr, wr, br, padding=1)
    ref.backward(dy)
    assert same_bits(S.conv3x3(x, wt, b), ref.detach())
    assert same_bits(S.conv3x3_dx(dy, wt), xr.grad)
    assert same_bits(S.conv3x3_dw(x, dy), wr.grad)
    assert same_bits(S.conv3x3_db(dy), br.grad)
    # the row layouts round-trip
    rows = S.nchw_to_rows(x)
    assert rows.shape == (B * h * w, ci) and same_bits(S.rows_to_nchw(rows, B, h, w), x)


def test_restatement_in_fp32_is_close():
    """The fp32 evaluation (the floor's yardstick) is the same function: a few ulps from fp64."""
    g = torch.Generator().manual_seed(3)
    x, wt, b = torch.randn(2, 64, 16, 16, generator=g), torch.randn(3, 64, 3, 3, generator=g), torch.randn(3, generator=g)
    y64 = S.conv3x3(x.double(), wt.double(), b.double())
    y32 = S.conv3x3(x, wt, b)
    assert y32.dtype == torch.float32 and (y32.double() - y64).abs().max() < 1e-4


# ------------------------------------------------------------------ perturbed variants are rejected
def _drop_tap(x, w, b, tap=5):
    w = w.clone()
    w.view(w.shape[0], w.shape[1], 9)[:, :, tap] = 0
    return S.conv3x3(x, w, b)


def _swap_hw(x, w, b):
    """The image indexed as w x h: rows of length h."""
    B, ci, h, wd = x.shape
    y = S.conv3x3(x.reshape(B, ci, wd, h), w, b)
    return y.reshape(B, w.shape[0], h, wd)


def _bleed(x, w, b):
    """No padding between the images of a batch: a border row reads the neighbouring image."""
    B, ci, h, wd = x.shape
    tall = x.permute(1, 0, 2, 3).reshape(1, ci, B * h, wd)
    y = S.conv3x3(tall, w, b)
    return y.reshape(w.shape[0], B, h, wd).permute(1, 0, 2, 3).contiguous()


@pytest.mark.parametrize("variant", [_drop_tap, _swap_hw, _bleed], ids=lambda f: f.__name__)
def test_exact_comparison_rejects_perturbations(variant):
    x, wt, b, _ = _case(3, 5, 7, 8, 3, seed=11)
    good = S.conv3x3(x, wt, b)
    assert same_bits(good, Fn.conv2d(x, wt, b, padding=1))
    bad = variant(x, wt, b)
    assert bad.shape == good.shape and not same_bits(bad, good)
    if variant is _swap_hw:  # invisible on a square image's shape, visible in its values
        xs = _case(2, 4, 4, 8, 3, seed=12)[0]
        assert same_bits(_swap_hw(xs, wt, b), S.conv3x3(xs, wt, b))  # h == w: the same function
    if variant is _bleed:  # only border rows differ
        diff = (bad != good).any(dim=1)
        assert not diff[:, 1:-1].any() and diff[:, [0, -1]].any()


# ------------------------------------------------------------------ host-side refusals
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
# A 16-byte aligned number standing in for device memory.  Every case below must be refused before any
# launch BY CONSTRUCTION: exactly one argument of an otherwise valid call is wrong and the expected
# code is a refusal, so nothing ever dereferences this address.  Add no case here that is meant to be
# accepted (a launch on it would fault on a machine with a GPU).
P = 0x7F0000001000


@pytest.fixture(scope="module")
def L():
    import encdiff_amd._lib as lib
    return lib


def _in_args(L, **kw):
    a = dict(batch=2, h=5, w=7, cin=3, cout=8, x=P, ldx=0, x_f32=1, weight=P, bias=P, y=P, ldy=8, y_f32=0)
    a.update(kw)
    return L.SmallConvArgs(**a)


def _out_args(L, **kw):
    a = dict(batch=2, h=5, w=7, cin=64, cout=3, x=P, ldx=64, x_f32=0, weight=P, bias=P, y=P, ldy=0, y_f32=1,
             dy=P, lddy=0, dy_f32=1, dx=P, lddx=64)
    a.update(kw)
    return L.SmallConvArgs(**a)


@pytest.mark.parametrize("kw,rc", [
    (dict(cin=5), ERR_SHAPE), (dict(cout=12, ldy=16), ERR_SHAPE), (dict(cout=72, ldy=72), ERR_SHAPE),
    (dict(ldy=12), ERR_SHAPE), (dict(x=None), ERR_ARG), (dict(y=P + 8), ERR_ARG), (dict(y=P + 2), ERR_ARG)],
    ids=str)
def test_input_conv_refusals(L, kw, rc):
    assert L.lib.encdiff_small_conv_fwd(C.byref(_in_args(L, **kw)), None) == rc


@pytest.mark.parametrize("kw,rc", [
    (dict(cout=4), ERR_SHAPE), (dict(cin=520, ldx=520), ERR_SHAPE), (dict(cin=12, ldx=16), ERR_SHAPE),
    (dict(x=None), ERR_ARG), (dict(ldx=68), ERR_ARG), (dict(ldx=65), ERR_ARG), (dict(x=P + 8), ERR_ARG),
    (dict(x=P + 2), ERR_ARG), (dict(x_f32=1), ERR_UNSUPPORTED), (dict(y_f32=0), ERR_UNSUPPORTED)], ids=str)
def test_output_conv_forward_refusals(L, kw, rc):
    """ldx % 8 and the 16-byte alignment of x: the kernels read 8 bf16 channels per 16-byte load."""
    assert L.lib.encdiff_small_conv_fwd(C.byref(_out_args(L, **kw)), None) == rc


@pytest.mark.parametrize("kw,rc", [
    (dict(dy_f32=0), ERR_UNSUPPORTED), (dict(cout=4), ERR_UNSUPPORTED), (dict(cin=12), ERR_UNSUPPORTED),
    (dict(cin=520), ERR_SHAPE), (dict(x=None), ERR_ARG), (dict(dy=None), ERR_ARG), (dict(lddx=68), ERR_ARG),
    (dict(lddx=67), ERR_ARG), (dict(dx=P + 8), ERR_ARG), (dict(dx=P + 2), ERR_ARG),
    # the weight gradient stages (cin + cout) x h x w floats in LDS: 67 x 625 x 4 B > 160 KiB
    (dict(dx=None, dweight=P, batch=1, h=25, w=25), ERR_SHAPE)], ids=str)
def test_output_conv_backward_refusals(L, kw, rc):
    """dx requested with a bf16 dy is unsupported; lddx % 8 and dx's alignment: 16-byte stores."""
    assert L.lib.encdiff_small_conv_bwd(C.byref(_out_args(L, **kw)), None) == rc
