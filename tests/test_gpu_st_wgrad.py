"""Per-element tests of the grouped weight gradients of the fused transformer blocks on the
MI355X: st_wgrad_kernel, st_wgrad_fold_kernel and the fold riding in the GroupNorm backward
(csrc/st_bwd.hip, csrc/stwg.h, csrc/norm.hip) against tests/stwg_restate.py in fp64.

The tests plan and launch through encdiff_amd._lib with a workspace of their own (as
ops.StWgrad.launch does), read kc / kb / kind back from the plan blob and assert that each case
reached the path it is named for: a change of ENCDIFF_STWG_KC or of the planner fails here
instead of silently losing coverage.

Exact mode: dY, X integers in [-3, 3], prior dW / db in [-64, 64], K <= 4352: every sum is an
integer below 9 * 4352 + 64 = 39,232 < 2^17, exact in fp32 in any order (MFMA accumulation, slab
fold, in-place add), so dW and db must equal the fp64 value cast to fp32 bit for bit.
Rounded mode: seeded randn rounded to bf16, fp32 rule per element against fp64, floor = 4 x max
|fp32 chunked restatement - fp64| measured on the device and printed.
Every dW (contiguous, and with ld_dw = N + 3 at first column 1) and db is a `Guard` view.

Kernel branch -> test
  st_wgrad_body, all eight (WM, WN) kinds of STWG_KINDS ................ test_exact[64-*] + [128-*]
  one stage (K = 32), three stages, one full chunk in place (K = 256) .. test_exact[*-32 / 96 / 256]
  short last chunk of one 32-token stage (K = 288, kb = 2) ............. test_exact[*-288]
  fold group wrap: kb = 9 (group 0 sums chunks 0 and 8), kb = 17 ....... test_exact[*-2080 / 4352]
  dY / X column slices (ld = width + 64, first column 8), ld_dw = N + 3
    in the in-place path and in the fold, db .......................... test_exact (strided pass)
  a group mixing one-chunk and multi-chunk problems (fold's lookup) .... test_mixed_k
  a workspace that forces the plan to double kc ........................ test_small_workspace
  encdiff_st_wgrad_launch_nofold + the fold in groupnorm_bwd ........... test_riding_fold
  ops.StWgrad (its own scratch workspace), with and without ride ....... test_riding_fold
  rounded inputs, per element, and run-to-run bits ..................... test_rounded
  the plan's refusals (no GPU needed) .................................. test_stwg_restate.py
"""
import ctypes as C

import pytest
import torch

import elementwise_restate as R
import stwg_restate as W
from test_abi import StWg  # the plan blob's problem record (stwg.h)
from test_gpu_elementwise import Guard, _gen, assert_f32_rule, rnd

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KC = 256  # the planner's default chunk (ENCDIFF_STWG_KC); asserted from the blob in every case
# (M, N, bias) of a c = 64 block's eight Linear layers, in the executor's order (unet.py, _st_bwd_fused):
# proj_out, ff.net.2, ff.net.0.proj, attn2.to_out, attn2.to_q (no bias), attn1.to_out, qkv (no bias), proj_in
SHAPES64 = [(64, 64, True), (64, 256, True), (512, 64, True), (64, 64, True), (64, 64, False), (64, 64, True),
            (192, 64, False), (64, 64, True)]
WS_FLOATS = 8 << 20  # 32 MiB: the c = 128 list at K = 4352 needs 17 x 327,680 + biases = 5.6 M floats


def shapes_of(c):
    return [(M * c // 64, N * c // 64, b) for M, N, b in SHAPES64]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd._lib as lib
    return lib


@pytest.fixture(scope="module")
def ws(L):
    return torch.empty(WS_FLOATS, device=dev)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ints(g, lo, hi, *shape, dtype=F32):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(dev)


class Case:
    """One problem list: operands (contiguous or column slices), prior values, Guards."""

    def __init__(self, shapes, Ks, exact, strided, seed):
        g = _gen(seed)
        self.items = []
        for (M, N, has_b), K in zip(shapes, Ks):
            if exact:
                dy, x = _ints(g, -3, 3, K, M, dtype=BF16), _ints(g, -3, 3, K, N, dtype=BF16)
                dw0, db0 = _ints(g, -64, 64, M, N), _ints(g, -64, 64, 1, M)
            else:
                # specials in X only: +-90 in both operands would meet in one product (8100) whose fp32
                # rounding would set the whole tensor's floor a thousand times above a typical element's
                dy, x = rnd(g, K, M, scale=0.1, dtype=BF16), rnd(g, K, N, dtype=BF16, specials=True)
                dw0, db0 = rnd(g, M, N), rnd(g, 1, M)
            if strided:  # column slices of wider buffers; dW at an odd row stride
                dyv = Guard(K, M, BF16, ld=M + 64, left=8, init=dy).view
                xv = Guard(K, N, BF16, ld=N + 64, left=8, init=x).view
                dw = Guard(M, N, F32, ld=N + 3, left=1, init=dw0)
            else:
                dyv, xv, dw = dy, x, Guard(M, N, F32, init=dw0)
            db = Guard(1, M, F32, init=db0) if has_b else None
            self.items.append(dict(dy=dy, x=x, dyv=dyv, xv=xv, dw=dw, db=db, dw0=dw0, db0=db0.view(-1) if has_b else None,
                                   M=M, N=N, K=K))

    def probs(self):
        """(dy, x, dw, db) views as ops.StWgrad.launch takes them."""
        return [(i["dyv"], i["xv"], i["dw"].view, None if i["db"] is None else i["db"].view.view(-1)) for i in self.items]

    def reset(self):
        for i in self.items:
            i["dw"].view.copy_(i["dw0"])
            if i["db"] is not None:
                i["db"].view.view(-1).copy_(i["db0"])

    def outputs(self):
        return [(i["dw"].view.clone(), None if i["db"] is None else i["db"].view.clone()) for i in self.items]

    def check(self, exact, kcs, what):
        for n, (i, kc) in enumerate(zip(self.items, kcs)):
            i["dw"].check()
            ev = lambda dt: W.wgrad_chunked(i["dy"], i["x"], i["dw0"], i["db0"], kc, dt)
            rw, rb = W.wgrad(i["dy"], i["x"], i["dw0"], i["db0"], F64)
            outs = [("dW", i["dw"].view, rw, 0)]
            if i["db"] is not None:
                i["db"].check()
                outs.append(("db", i["db"].view.view(-1), rb, 1))
            for name, got, ref, k in outs:
                tag = f"{what} problem {n} ({i['M']}x{i['N']}, K={i['K']}) {name}"
                if exact:
                    want = ref.to(F32)
                    bad = (R.bits(got.contiguous()) != R.bits(want)).flatten().nonzero()
                    assert bad.numel() == 0, (f"{tag}: {bad.numel()} elements differ, first at {int(bad[0])}: got "
                                              f"{got.flatten()[int(bad[0])].item()} want {want.flatten()[int(bad[0])].item()}")
                else:
                    assert_f32_rule(got, ref, ev(F32)[k], tag)


def plan(L, case, ws, ws_floats):
    """encdiff_st_wgrad_plan on the case's views: (host blob, device blob, header, problem records)."""
    pr = case.probs()
    arr = (L.WgradProb * len(pr))(*[
        L.WgradProb(dy=dy.data_ptr(), ld_dy=dy.stride(0), x=x.data_ptr(), ld_x=x.stride(0), dw=dw.data_ptr(),
                    ld_dw=dw.stride(0), db=None if db is None else db.data_ptr(), M=dy.shape[1], N=x.shape[1],
                    K=dy.shape[0]) for dy, x, dw, db in pr])
    nb = C.c_long(0)
    L.check(L.lib.encdiff_st_wgrad_plan(arr, len(pr), ws.data_ptr(), ws_floats, None, 0, C.byref(nb)), "plan size")
    host = (C.c_longlong * ((nb.value + 7) // 8))()
    L.check(L.lib.encdiff_st_wgrad_plan(arr, len(pr), ws.data_ptr(), ws_floats, C.addressof(host), C.sizeof(host),
                                        C.byref(nb)), "plan")
    hdr = list((C.c_int * 4).from_buffer(host))
    assert hdr[0] == 0x53545747 and hdr[1] == len(pr)
    recs = (StWg * len(pr)).from_address(C.addressof(host) + 64)
    for p in recs:  # the slabs lie inside the workspace this test owns
        if p.kb > 1:
            lo = (p.slab - ws.data_ptr()) // 4
            assert 0 <= lo and lo + p.kb * p.M * (p.N + 1) <= ws_floats
    blob = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
    return host, blob, hdr, recs


def launch(L, host, blob):
    L.check(L.lib.encdiff_st_wgrad_launch(C.addressof(host), blob.data_ptr(), _stream()), "encdiff_st_wgrad_launch")
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", [32, 96, 256, 288, 2080, 4352])
@pytest.mark.parametrize("c", [64, 128])
def test_exact(L, ws, c, K):
    """The eight weight gradients of a c = 64 / 128 block, exact mode, operands contiguous and then as
    column slices with dW at ld_dw = N + 3.  K = 32: one stage; 96: three; 256: one whole chunk added
    in place (no slab, no fold); 288: two chunks, the second a single stage; 2080: nine chunks (fold
    group 0 sums chunks 0 and 8) with a 32-token last chunk; 4352: seventeen (groups 0 wraps twice).
    The c = 64 list plans kinds 0-3, the c = 128 list kinds 4-7 (asserted from the blob).
    Catches: a stage or a chunk dropped or taken twice, the last short chunk read at full length,
    chunk 8 (or 16) left out of the fold, a slab of problem i folded into problem j, a bias taken
    from another 64-column block of dY or summed over the block columns more than once, prior dW / db
    overwritten, a row of dW written at stride N when ld_dw != N (the Guard and the values)."""
    kinds = set()
    for strided in (False, True):
        case = Case(shapes_of(c), [K] * 8, True, strided, seed=c + K)
        host, blob, hdr, recs = plan(L, case, ws, WS_FLOATS)
        for p in recs:
            assert (p.kc, p.kb) == (min(KC, K), -(-K // KC)), (p.kc, p.kb)
            kinds.add(p.kind)
        assert (hdr[3] > 0) == (K > KC)
        launch(L, host, blob)
        case.check(True, [p.kc for p in recs], f"c={c} K={K} strided={int(strided)}")
    assert kinds == ({0, 1, 2, 3} if c == 64 else {4, 5, 6, 7})


def test_mixed_k(L, ws):
    """One group with K = 256, 2080, 32: a one-chunk problem before and after a nine-chunk one, so
    consecutive problems share a fold0 and the fold's problem lookup must pick the middle one."""
    shapes = [(64, 64, True), (192, 64, True), (64, 256, True)]
    for strided in (False, True):
        case = Case(shapes, [256, 2080, 32], True, strided, seed=77)
        host, blob, hdr, recs = plan(L, case, ws, WS_FLOATS)
        assert [p.kb for p in recs] == [1, 9, 1]
        assert recs[0].fold0 == recs[1].fold0 == 0 and recs[2].fold0 == hdr[3] > 0
        launch(L, host, blob)
        case.check(True, [p.kc for p in recs], f"mixed K strided={int(strided)}")


def _need(shapes, K, kc):
    kb = -(-K // kc)
    return sum((kb * M * N + (kb * M if b else 0) + 31) & ~31 for M, N, b in shapes)


def test_small_workspace(L, ws):
    """The c = 64 list at K = 2080 with a workspace that holds the five slabs of kc = 512 but not the
    nine of kc = 256: the plan doubles kc (asserted), and the results are still exact."""
    shapes = shapes_of(64)
    small = _need(shapes, 2080, 512)
    assert small < _need(shapes, 2080, KC)
    case = Case(shapes, [2080] * 8, True, True, seed=88)
    host, blob, hdr, recs = plan(L, case, ws, small)
    assert all(p.kc == 512 and p.kb == 5 for p in recs), [(p.kc, p.kb) for p in recs]
    launch(L, host, blob)
    case.check(True, [p.kc for p in recs], "small workspace")


def test_riding_fold(L, ws):
    """The K = 2080 c = 64 list through ops.StWgrad().launch(ride=True): only the weight-gradient grid
    is launched, the fold runs as extra workgroups of a small GroupNorm backward (B = 2, 8 x 8,
    c = 64).  dW and db are exact, and dx and the dgamma / dbeta partials of the GroupNorm are bit
    for bit those of the same call without a fold."""
    from encdiff_amd import ops
    g = _gen(99)
    B, hw, c = 2, 64, 64
    gg = ops.Geom(B, 8, 8)
    xg = (rnd(g, B * hw, c) + 0.3).to(BF16)
    gam, bet = 1 + 0.1 * rnd(g, c), 0.1 * rnd(g, c)
    yg, st = torch.empty_like(xg), torch.empty(B, 32, 2, device=dev)
    ops.groupnorm_fwd(xg, gg, gam, bet, yg, st, 1e-6, False)
    dyg = rnd(g, B * hw, c, scale=0.1, dtype=BF16)
    case = Case(shapes_of(64), [2080] * 8, True, True, seed=99)
    res = []
    # the planner owns the device plan the queued kernels (and the riding fold) read: it must outlive them
    sw = ops.StWgrad()
    for ride in (False, True):
        case.reset()
        dx = Guard(B * hw, c, BF16)
        dgp, dbp = Guard(B, c, F32), Guard(B, c, F32)
        fold = sw.launch(case.probs(), ride=ride)
        assert (fold is not None) == ride
        ops.groupnorm_bwd(xg, gg, gam, bet, st, 1e-6, False, dyg, dx.view, dgp.view, dbp.view, fold=fold)
        torch.cuda.synchronize()
        # the plan ops.StWgrad made in its own workspace: nine chunks of 256 per problem, a fold to ride
        (host, blob), = sw._plans.values()
        hdr = list((C.c_int * 4).from_buffer(host))
        recs = (StWg * hdr[1]).from_address(C.addressof(host) + 64)
        assert hdr[0] == 0x53545747 and hdr[1] == 8 and hdr[3] > 0
        assert all((p.kc, p.kb) == (KC, 9) for p in recs), [(p.kc, p.kb) for p in recs]
        if ride:
            assert fold == (blob.data_ptr(), hdr[3])
        for q in (dx, dgp, dbp):
            q.check()
        case.check(True, [p.kc for p in recs], f"ride={int(ride)}")
        res.append((dx.buf.clone(), dgp.buf.clone(), dbp.buf.clone()))
    for a, b in zip(*res):
        assert R.same_bits(a, b)


@pytest.mark.parametrize("c", [64, 128])
def test_rounded(L, ws, c):
    """Each list once at K = 2080 on randn inputs rounded to bf16 (dY scaled by 0.1; X with +-0, +-30,
    +-90 and bf16's smallest normals at both ends), strided: per element within
    floor + 2^-22 |ref| of fp64, the floor from the chunked restatement in fp32 (the plan's chunking
    and the fold's order), and the same bits from a second launch (slabs folded in a fixed order, no
    atomics).
    Measured on the MI355X over the eight problems, floor / worst |out - ref|: c = 64: dW 2.9e-5 ..
    8.4e-5 / 5.8e-6 .. 1.1e-5, db 2.4e-6 .. 5.8e-6 / 6.0e-7 .. 1.5e-6; c = 128: dW 4.4e-5 .. 8.0e-5 /
    4.9e-6 .. 1.2e-5, db 2.6e-6 .. 4.9e-6 / 6.6e-7 .. 1.2e-6."""
    case = Case(shapes_of(c), [2080] * 8, False, True, seed=5 * c)
    host, blob, hdr, recs = plan(L, case, ws, WS_FLOATS)
    launch(L, host, blob)
    case.check(False, [p.kc for p in recs], f"rounded c={c}")
    first = case.outputs()
    case.reset()
    launch(L, host, blob)
    for (w1, b1), (w2, b2) in zip(first, case.outputs()):
        assert R.same_bits(w1, w2) and (b1 is None or R.same_bits(b1, b2))
