"""CPU tests of tests/stwg_restate.py (the reference of tests/test_gpu_st_wgrad.py) and of the
host-side refusals of encdiff_st_wgrad_plan.

Exact mode: dY, X integers in [-3, 3], prior dW / db in [-64, 64], K <= 4352: every sum is an
integer below 9 * 4352 + 64 < 2^17, exact in any order, so the plain and the chunked restatement
and torch.matmul must agree bit for bit, and three deliberately wrong variants must not.  The plan
call needs no GPU: its refusals are checked by return code on pointers that are never dereferenced."""
import ctypes as C

import pytest
import torch

import stwg_restate as W
from elementwise_restate import same_bits

F32, F64 = torch.float32, torch.float64


def _case(K, M, N, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(F64)
    return r(-3, 3, K, M), r(-3, 3, K, N), r(-64, 64, M, N), r(-64, 64, M)


@pytest.mark.parametrize("K", [32, 96, 256, 288, 2080, 4352])
@pytest.mark.parametrize("M,N", [(64, 64), (192, 64), (64, 256)])
def test_plain_chunked_and_matmul_agree(K, M, N):
    dy, x, dw0, db0 = _case(K, M, N, seed=K + M + N)
    dw, db = W.wgrad(dy, x, dw0, db0, F64)
    assert same_bits(dw, dw0 + torch.matmul(dy.t(), x)) and same_bits(db, db0 + dy.sum(0))
    for kc in (256, 512, 32):
        cw, cb = W.wgrad_chunked(dy, x, dw0, db0, kc, F64)
        assert same_bits(cw, dw) and same_bits(cb, db), kc
    # in fp32 too (the sums stay below 2^24), and without a bias
    cw32, none = W.wgrad_chunked(dy, x, dw0, None, 256, F32)
    assert none is None and same_bits(cw32, dw.to(F32))


def test_chunks_and_fold_order():
    assert W.chunks(288, 256) == [(0, 256), (256, 288)] and W.chunks(256, 256) == [(0, 256)]
    assert len(W.chunks(2080, 256)) == 9 and len(W.chunks(4352, 256)) == 17
    # the fold's order, visible in fp32 on values that do not add exactly: group 0 = (p0 + p8) first
    parts = [torch.tensor([v], dtype=F32) for v in (2.0 ** 24, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)]
    g0 = torch.tensor([2.0 ** 24], dtype=F32) + 1.0  # p8 is lost in group 0
    want = g0
    for _ in range(7):
        want = want + 1.0
    assert same_bits(W.fold(parts), want) and W.fold(parts).item() != float(2 ** 24 + 8)


def _perturbed(dy, x, dw0, db0, kc, what):
    spans = W.chunks(dy.shape[0], kc)
    if what == "last_stage_dropped":
        spans[-1] = (spans[-1][0], spans[-1][1] - 32)
    ws, bs = W.slabs(dy, x, spans, F64)
    if what == "chunk8_skipped":
        ws[8], bs[8] = torch.zeros_like(ws[8]), torch.zeros_like(bs[8])
    if what == "bias_wrong_block":
        bs = W.slabs(torch.roll(dy, 64, 1), x, spans, F64)[1]
    return dw0 + W.fold(ws), db0 + W.fold(bs)


@pytest.mark.parametrize("what", ["last_stage_dropped", "chunk8_skipped", "bias_wrong_block"])
def test_exact_comparison_rejects_perturbations(what):
    dy, x, dw0, db0 = _case(2080, 192, 64, seed=5)
    dw, db = W.wgrad(dy, x, dw0, db0, F64)
    ok_w, ok_b = W.wgrad_chunked(dy, x, dw0, db0, 256, F64)
    assert same_bits(ok_w, dw) and same_bits(ok_b, db)
    bad_w, bad_b = _perturbed(dy, x, dw0, db0, 256, what)
    if what == "bias_wrong_block":
        assert same_bits(bad_w, dw) and not same_bits(bad_b, db)
    else:
        assert not same_bits(bad_w, dw) and not same_bits(bad_b, db)


# ------------------------------------------------------------------ host-side refusals of the plan
ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
P = 0x7F0000001000  # stands in for device memory: the plan call is host arithmetic, it never dereferences it


def _prob(L, **kw):
    a = dict(dy=P, ld_dy=64, x=P + (1 << 24), ld_x=64, dw=P + (2 << 24), ld_dw=64, db=P + (3 << 24), M=64, N=64, K=64)
    a.update(kw)
    return L.WgradProb(**a)


def _plan(L, probs, n=None):
    arr = (L.WgradProb * max(len(probs), 1))(*probs)
    nb = C.c_long(0)
    return L.lib.encdiff_st_wgrad_plan(arr, len(probs) if n is None else n, P + (1 << 30), 1 << 24, None, 0, C.byref(nb))


@pytest.mark.parametrize("kw,rc", [
    ({}, 0), (dict(M=96, ld_dy=96), ERR_SHAPE), (dict(N=96, ld_x=96, ld_dw=96), ERR_SHAPE), (dict(K=48), ERR_SHAPE),
    (dict(K=0), ERR_SHAPE), (dict(ld_dw=63), ERR_SHAPE), (dict(ld_dw=67), 0), (dict(ld_dy=68), ERR_ARG),
    (dict(dy=P + 8), ERR_ARG), (dict(x=P + 8), ERR_ARG), (dict(ld_x=68), ERR_ARG), (dict(dw=None), ERR_ARG),
    (dict(M=128, ld_dy=128), ERR_UNSUPPORTED), (dict(N=128, ld_x=128, ld_dw=128), ERR_UNSUPPORTED)], ids=str)
def test_plan_refusals(kw, rc):
    """M, N multiples of 64, K a positive multiple of 32, ld_dw >= N (ld_dw = N + 3 is accepted: dW is
    written by scalars), 16-byte aligned bf16 operands with row strides that are multiples of 8, and
    the two shapes no block kind serves: (M, N) = (128, 64) and (64, 128)."""
    import encdiff_amd._lib as L
    assert _plan(L, [_prob(L, **kw)]) == rc


def test_plan_refuses_problem_counts():
    import encdiff_amd._lib as L
    assert _plan(L, [_prob(L)] * 16) == 0
    assert _plan(L, [_prob(L)] * 17) == ERR_ARG
    assert _plan(L, [_prob(L)], n=0) == ERR_ARG
