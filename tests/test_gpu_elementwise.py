"""Per-element tests of the memory-bound step kernels on the MI355X: csrc/elementwise.hip, the
layout kernels of csrc/bn.hip and the elementwise / embedding / layout kernels of csrc/fp32.hip.

Whole-tensor rel-L2 cannot see a wrong last 16-byte vector, a skipped tail or one bad element in
4096, so these tests compare per element (tests/elementwise_restate.py):
  * data movement is bitwise (`same_bits`);
  * bf16-output arithmetic: |out - ref64| <= 2^-7 |ref64| + floor;
  * fp32 outputs: |out - ref64| <= floor + 2^-22 |ref64|;
    floor = 4 x the largest |torch fp32 evaluation - fp64| on the case's own inputs (measured at run
    time on the device; the values seen are quoted in the docstrings);
  * every output is a view inside a larger sentinel-filled buffer whose other bytes must not change.

Kernel branch -> test
  ew_kernel: each of the ten ops, accumulate 0 / 1, strided rows ....... test_ew_bf16
  ew_kernel: grid-stride loop (16400 x 512: 1,049,600 vectors) .......... test_ew_bf16[..-16400x512]
  ew_kernel: GEGLU_BWD honours accumulate (fixed here) .................. test_ew_bf16[geglu_bwd-..]
  ew_kernel: RESAMPLE / RESAMPLE_BWD, DOWN2 / UP2, 1x1, non-square ...... test_ew_bf16_resample
  ew_f32_kernel: eight ops, cols 1 / 5 / 72, accumulate, strided ........ test_ew_f32
  ew_f32_kernel: grid-stride loop (8200 x 257) .......................... test_ew_f32[..-8200x257]
  ed_elementwise_f32: ops 8 / 9 refused ................................. test_ew_f32_rejects_conversions
  nchw_to_rows_kernel: padding, ld > cpad, stride loop (1.31 M pixels) .. test_nchw_to_rows
  nchw_to_rows_kernel: split [hi | lo | hi] ............................. test_nchw_to_rows_split3
  nchw_rows_f32_kernel: dir 0 / 1, c < cpad, ld > cpad, stride loop ..... test_nchw_rows_f32
  pack_kernel: kind 0 vector path + stride loop, the three scalar-path
    conditions, scalar stride loop, kinds 1-6, job gaps ................. test_pack_weights_table
  adamw_ema_kernel: mirror / no mirror, ema None / n / n - 100 - r,
    ema_n % 4 != 0 tail lane, stride loop (n = 4,194,316), two ranges ... test_adamw_ema_mirror
  ParamArena.enable_ema: storage rounded to 4 floats .................... test_arena_ema_storage_rounded
  l1_kernel: fold loop batch > 256, per % 256 != 0, lsw, grad NULL, ties  test_l1_loss
  qsample_kernel: plain / scaled, stride loop, t = 0 / 999 .............. test_q_sample
  ddim_kernel: noise NULL, pred_x0 NULL, stride loop .................... test_ddim_step
  ddim_indexed_kernel + index_dec_kernel ................................ test_ddim_step_indexed
  temb_kernel / temb_f32_kernel ......................................... test_timestep_embedding
  reduce_partials_kernel: 4-row unrolled loop (rows > 24), tails ........ test_reduce_partials
  grad_fold_kernel: padding channels, db / gb, refusals ................. test_grad_fold
  gather_u8_kernel: byte-wise staging, 16-byte staging, id clamp ........ test_gather_images_u8_small
  bn_stats / bn_apply: x_f32, y_split, encdiff_batchnorm_apply .......... test_batchnorm_forms
  small_conv_in_fwd / out_fwd / out_fwd_lanes / out_dgrad / wgrad ....... tests/test_gpu_small_conv.py
  step_prologue_kernel: Philox stream, t, noise tails, zero jobs ........ tests/test_gpu_step_prologue.py
"""
import ctypes
import math

import pytest
import torch

import elementwise_restate as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -1232.0  # exact in bf16 and fp32
SPECIALS = [0.0, -0.0, 30.0, -30.0, 90.0, -90.0, 2.0 ** -126, -(2.0 ** -125), 1.5 * 2.0 ** -126]


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    return ops


@pytest.fixture(scope="module")
def L():
    import encdiff_amd._lib as lib
    return lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape, scale=1.0, dtype=F32, specials=False, tiny=True):
    """Seeded on the host (the same inputs on every machine), `randn * scale`; specials: 0, -0, +-30,
    +-90 and (tiny) values near bf16's smallest normal at the first and the last positions."""
    x = torch.randn(*shape, generator=g) * scale
    if specials:
        sp = SPECIALS if tiny else SPECIALS[:6]  # 0.25 x a smallest normal would be subnormal
        f = x.view(-1)
        k = min(len(sp), f.numel())
        f[:k] = torch.tensor(sp[:k])
        if f.numel() >= 2 * len(sp):
            f[-len(sp):] = torch.tensor(sp)
    return x.to(dtype).to(dev)


class Guard:
    """A [rows][cols] view (row stride ld, first column at `left`) inside a flat sentinel-filled
    buffer with `pad` sentinels in front and behind; check() proves every element outside the view
    is bitwise unchanged.  ld / left choose the row stride and first column themselves (odd strides,
    misaligned views); fill: what the buffer holds around the view."""

    def __init__(self, rows, cols, dtype, strided=False, init=None, pad=64, ld=None, left=None, fill=SENT):
        dld, dleft = (cols + 24, 8) if strided else (cols, 0)
        ld, left = (dld if ld is None else ld), (dleft if left is None else left)
        assert left + cols <= ld
        self.geom = ((rows, cols), (ld, 1), pad + left)
        self.buf = torch.full((pad + rows * ld + pad,), fill, dtype=dtype, device=dev)
        self.view = self.buf.as_strided(*self.geom)
        if init is not None:
            self.view.copy_(init)
        self.before = self.buf.clone()

    def check(self):
        after = self.buf.clone()
        after.as_strided(*self.geom).copy_(self.before.as_strided(*self.geom))
        assert R.same_bits(after, self.before), "wrote outside the logical output"


def place(x, strided):
    """x as a contiguous tensor or as a column slice of a wider buffer (offset 8, stride + 24)."""
    if not strided:
        return x.contiguous()
    return Guard(x.shape[0], x.shape[1], x.dtype, strided=True, init=x).view


def assert_bf16_rule(out, ref64, t32, what):
    floor = R.floor_of(t32, ref64)
    ex, i, worst = R.bf16_excess(out, ref64, floor)
    print(f"{what}: floor {floor:.3e} max|out-ref| {worst:.3e} excess {ex:.3e}")
    assert ex <= 0, f"{what}: element {i} exceeds 2^-7|ref| + {floor:.3e} by {ex:.3e}"


def assert_f32_rule(out, ref64, t32, what):
    floor = R.floor_of(t32, ref64)
    ex, i, worst = R.f32_excess(out, ref64, floor)
    print(f"{what}: floor {floor:.3e} max|out-ref| {worst:.3e} excess {ex:.3e}")
    assert ex <= 0, f"{what}: element {i} exceeds {floor:.3e} + 2^-22|ref| by {ex:.3e}"


# ====================================================================== 1. bf16 encdiff_elementwise
EW_NAMES = ["copy", "silu", "silu_bwd", "geglu", "geglu_bwd", "add", "f32_to_bf16", "bf16_to_f32"]
EW_OPS = {"copy": 0, "silu": 1, "silu_bwd": 2, "geglu": 3, "geglu_bwd": 4, "add": 5, "f32_to_bf16": 8,
          "bf16_to_f32": 9}


def _ew_eval(name, x, x2, dt):
    """The op on the (already rounded) inputs, evaluated in dtype dt."""
    x = x.to(dt)
    x2 = None if x2 is None else x2.to(dt)
    if name in ("copy", "f32_to_bf16", "bf16_to_f32"):
        return x
    if name == "silu":
        return R.silu(x)
    if name == "silu_bwd":
        return x2 * R.silu_grad(x)
    if name == "geglu":
        return R.geglu(x)
    if name == "geglu_bwd":
        return R.geglu_bwd(x, x2)
    if name == "add":
        return x + x2
    raise ValueError(name)


def _ew_case(O, name, rows, cols, strided, acc, dtype, seed):
    g = _gen(seed)
    in_dt = F32 if (dtype == F32 or name == "f32_to_bf16") else BF16
    out_dt = F32 if (dtype == F32 or name == "bf16_to_f32") else BF16
    xc = 2 * cols if name in ("geglu", "geglu_bwd") else cols
    yc = 2 * cols if name == "geglu_bwd" else cols
    x = place(rnd(g, rows, xc, scale=3.0, dtype=in_dt, specials=True), strided)
    x2 = place(rnd(g, rows, cols, scale=3.0, dtype=in_dt), strided) if name in ("silu_bwd", "geglu_bwd", "add") else None
    prev = rnd(g, rows, yc, scale=3.0, dtype=out_dt)
    y = Guard(rows, yc, out_dt, strided=strided, init=prev)
    fn = O.ew_f32 if dtype == F32 else O.ew
    fn(EW_OPS[name], x, y.view, x2=x2, rows=rows, cols=cols, accumulate=bool(acc))
    torch.cuda.synchronize()
    y.check()
    what = f"{name} {rows}x{cols} strided={int(strided)} acc={acc}"
    moves = name in ("copy", "f32_to_bf16", "bf16_to_f32")
    if moves and not acc:
        assert R.same_bits(y.view.contiguous(), x.to(out_dt).contiguous()), what
        return
    if moves and acc and out_dt == F32:  # one exactly rounded fp32 add
        assert R.same_bits(y.view.contiguous(), prev + x.float()), what
        return
    ref = _ew_eval(name, x, x2, F64)
    t32 = _ew_eval(name, x, x2, F32)
    if acc:
        ref, t32 = ref + prev.double(), t32 + prev.float()
    (assert_f32_rule if out_dt == F32 else assert_bf16_rule)(y.view, ref, t32, what)


@pytest.mark.parametrize("rows,cols", [(1, 8), (37, 24), (1000, 72), (16400, 512)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("name", EW_NAMES)
def test_ew_bf16(O, name, rows, cols):
    """Every bf16 op, contiguous and as column slices, accumulate 0 and 1.  Catches: the last
    8-element vector of a row (or of the capped grid's second pass at 16400 x 512) dropped; a row
    stride taken for the column count; GEGLU halves swapped; `accumulate` ignored (GEGLU_BWD did,
    fixed with this test) or applied before the rounding; a conversion that truncates instead of
    rounding to nearest even; writes past a strided row's last column.
    Largest floors measured on the MI355X for these inputs (4 x torch fp32 vs fp64; the inputs
    reach +-90, so they are a few fp32 ulps of ~100): silu 4.5e-6 (7.8e-6 accumulating), silu_bwd
    2.4e-5 (2.7e-5), geglu 5.1e-5 (4.3e-5), geglu_bwd 6.8e-5 (6.7e-5), add 1.9e-6 (2.4e-6),
    copy + accumulate 1.9e-6, f32_to_bf16 + accumulate 3.8e-6."""
    for strided in (False, True):
        for acc in (0, 1):
            _ew_case(O, name, rows, cols, strided, acc, BF16, seed=1000 + rows + 7 * acc + int(strided))


def _resample_case(O, L, dtype, bwd, mode, b, h, w, cols, strided, acc, seed):
    """(b, h, w): the FORWARD op's output geometry."""
    g = _gen(seed)
    dt = dtype
    down = mode == L.RESAMPLE_DOWN2
    big, small = (b, 2 * h, 2 * w), (b, h // 2, w // 2)
    if not bwd:
        src, out = (big if down else small), (b, h, w)
    else:  # adjoint: input at the forward's output geometry, output at the forward's source geometry
        src, out = (b, h, w), (big if down else small)
    pix = lambda s: s[0] * s[1] * s[2]
    x = place(rnd(g, pix(src), cols, scale=3.0, dtype=dt, specials=True, tiny=False), strided)
    prev = rnd(g, pix(out), cols, scale=3.0, dtype=dt)
    y = Guard(pix(out), cols, dt, strided=strided, init=prev)
    fn = O.ew_f32 if dt == F32 else O.ew
    fn(L.EW_RESAMPLE_BWD if bwd else L.EW_RESAMPLE, x, y.view, accumulate=bool(acc), resample=mode,
       g=O.Geom(*out))
    torch.cuda.synchronize()
    y.check()

    def ev(d):
        xs = x.to(d)
        if not bwd:
            return R.avgpool2(xs, *out) if down else R.nearest2(xs, *out)
        return R.avgpool2_adjoint(xs, *out) if down else R.nearest2_adjoint(xs, *out)
    what = f"resample bwd={int(bwd)} mode={mode} out={out} cols={cols} strided={int(strided)} acc={acc}"
    if not acc and (down == bwd):  # nearest x2, and the 0.25 dy adjoint of the average: exact
        assert R.same_bits(y.view.contiguous(), ev(F32).to(dt).contiguous()), what
        return
    ref, t32 = ev(F64), ev(F32)
    if acc:
        ref, t32 = ref + prev.double(), t32 + prev.float()
    (assert_f32_rule if dt == F32 else assert_bf16_rule)(y.view, ref, t32, what)


@pytest.mark.parametrize("mode,shape", [("down2", (3, 8, 8)), ("down2", (2, 1, 1)), ("down2", (2, 6, 4)),
                                        ("up2", (3, 8, 8)), ("up2", (2, 2, 2)), ("up2", (2, 6, 4))], ids=str)
@pytest.mark.parametrize("bwd", [0, 1])
def test_ew_bf16_resample(O, L, bwd, mode, shape):
    """RESAMPLE and RESAMPLE_BWD, both modes, square / 1x1 / 2x2 / non-square (h != w), with and
    without accumulate, contiguous and strided.  Catches: h and w exchanged (invisible on square
    images), the child row offset 2w taken as w, a missing 0.25, the batch stride of the source
    taken at the output size, accumulate ignored.  Floors measured on the MI355X: 8.9e-8 for the average, 0 for the sum of four."""
    m = L.RESAMPLE_DOWN2 if mode == "down2" else L.RESAMPLE_UP2
    b, h, w = shape
    for strided in (False, True):
        for acc in (0, 1):
            _resample_case(O, L, BF16, bwd, m, b, h, w, 24, strided, acc, seed=2000 + h * w + acc)


# ====================================================================== 2. fp32 encdiff_elementwise
F32_NAMES = ["copy", "silu", "silu_bwd", "geglu", "geglu_bwd", "add"]


@pytest.mark.parametrize("rows,cols", [(37, 1), (37, 5), (37, 72), (8200, 257)], ids=lambda v: str(v))
@pytest.mark.parametrize("name", F32_NAMES)
def test_ew_f32(O, name, rows, cols):
    """The fp32 kernel's pointwise ops at cols 1 / 5 / 72 and over the 8192-workgroup cap
    (8200 x 257 = 2,107,400 elements), strided, accumulate on every op (GEGLU_BWD included).
    Catches: the stride loop's second pass dropped, the gate half read at column ld instead of
    cols, accumulate applied to one GEGLU_BWD half only.  Largest floors measured on the MI355X: silu 5.0e-6
    (1.2e-5 accumulating), silu_bwd 2.9e-5 (2.8e-5), geglu 1.1e-4 (5.2e-5), geglu_bwd 5.5e-5
    (9.5e-5), add 1.1e-5 (2.3e-5); copy is bitwise."""
    for strided in (False, True):
        for acc in (0, 1):
            _ew_case(O, name, rows, cols, strided, acc, F32, seed=3000 + rows + cols + acc)


@pytest.mark.parametrize("cols", [1, 5, 72, 257])
@pytest.mark.parametrize("mode", ["down2", "up2"])
@pytest.mark.parametrize("bwd", [0, 1])
def test_ew_f32_resample(O, L, bwd, mode, cols):
    """fp32 RESAMPLE / RESAMPLE_BWD on a non-square image; cols = 257 runs (2, 50, 82) pixels, over
    the grid cap.  Catches the same index mistakes as the bf16 test.  Largest floors measured on the MI355X: average 8.6e-6, its adjoint
    3.8e-6 (accumulating; bitwise otherwise), nearest 1.5e-5 (accumulating), sum of four 3.1e-5."""
    m = L.RESAMPLE_DOWN2 if mode == "down2" else L.RESAMPLE_UP2
    b, h, w = (2, 50, 82) if cols == 257 else (2, 6, 4)
    for strided in (False, True):
        for acc in (0, 1):
            _resample_case(O, L, F32, bwd, m, b, h, w, cols, strided, acc, seed=3500 + cols + acc)


@pytest.mark.parametrize("op", [8, 9])
def test_ew_f32_rejects_conversions(O, L, op):
    """F32_TO_BF16 / BF16_TO_F32 with dtype = F32 are refused before any launch."""
    x = torch.zeros(4, 8, device=dev)
    y = torch.full((4, 8), SENT, device=dev)
    with pytest.raises(L.HipError):
        O.ew_f32(op, x, y)
    torch.cuda.synchronize()
    assert (y == SENT).all()


# ====================================================================== 3. layout kernels
@pytest.mark.parametrize("B,C,HW,cpad,ld", [(2, 3, 16, 8, 8), (3, 4, 100, 8, 24), (1, 11, 7, 16, 16),
                                            (5, 3, 262144, 8, 8)])
def test_nchw_to_rows(O, L, B, C, HW, cpad, ld):
    """fp32 NCHW -> bf16 rows, bitwise.  Catches: padding channels left stale instead of zeroed,
    columns cpad..ld overwritten, the second 8-channel block (C = 11) reading channel c0 + k of the
    wrong image, pixels past the capped grid's first pass (1.31 M) skipped."""
    x = rnd(_gen(B * HW), B, C, HW, scale=3.0, specials=True)
    n = B * HW
    buf = torch.full((64 + n * ld + 64,), SENT, dtype=BF16, device=dev)
    y = buf[64:64 + n * ld].view(n, ld)
    L.check(L.lib.encdiff_nchw_to_rows(x.data_ptr(), B, C, HW, cpad, y.data_ptr(), ld, _stream()), "nchw_to_rows")
    torch.cuda.synchronize()
    exp = torch.full_like(buf, SENT)
    exp[64:64 + n * ld].view(n, ld)[:, :cpad] = R.nchw_to_rows_ref(x, cpad)
    assert R.same_bits(buf, exp)


@pytest.mark.parametrize("B,C,HW,cpad,ld", [(2, 3, 16, 8, 24), (3, 4, 100, 8, 40), (1, 11, 7, 16, 48)])
def test_nchw_to_rows_split3(O, L, B, C, HW, cpad, ld):
    """Split-bf16 rows [bf16(x) | bf16(x - hi) | hi], bitwise.  Catches: hi / lo blocks swapped, lo
    formed from the unrounded value (all zero), the third block placed at 2 * ld or 2 * C."""
    x = rnd(_gen(B + HW), B, C, HW, scale=3.0, specials=True)
    n = B * HW
    buf = torch.full((64 + n * ld + 64,), SENT, dtype=BF16, device=dev)
    y = buf[64:64 + n * ld].view(n, ld)
    L.check(L.lib.encdiff_nchw_to_rows_split3(x.data_ptr(), B, C, HW, cpad, y.data_ptr(), ld, _stream()), "split3")
    torch.cuda.synchronize()
    exp = torch.full_like(buf, SENT)
    exp[64:64 + n * ld].view(n, ld)[:, :3 * cpad] = R.nchw_to_rows_ref(x, cpad, split=True)
    assert R.same_bits(buf, exp)


@pytest.mark.parametrize("B,C,HW,cpad,ld", [(2, 3, 16, 8, 12), (3, 5, 37, 8, 8), (2, 3, 140000, 8, 12)])
def test_nchw_rows_f32(O, L, B, C, HW, cpad, ld):
    """fp32 NCHW <-> rows in both directions with c < cpad and ld > cpad; 2 x 140000 x 8 =
    2,240,000 elements is over the 8192-workgroup cap.  Catches: dir 1 writing cpad channels' worth
    of NCHW (past the tensor), padding not zeroed, columns cpad..ld touched, a lost second pass."""
    x = rnd(_gen(HW), B, C, HW, scale=3.0, specials=True)
    n = B * HW
    buf = torch.full((64 + n * ld + 64,), SENT, dtype=F32, device=dev)
    y = buf[64:64 + n * ld].view(n, ld)
    O.nchw_rows_f32(x, B, C, HW, cpad, y, ld, to_rows=True)
    torch.cuda.synchronize()
    exp = torch.full_like(buf, SENT)
    exp[64:64 + n * ld].view(n, ld)[:, :cpad] = R.nchw_rows_f32_ref(x, cpad)
    assert R.same_bits(buf, exp)
    # back: the padding channels of the rows hold a value dir 1 must not copy anywhere
    y[:, C:cpad] = 7.0
    back = torch.full((64 + B * C * HW + 64,), SENT, dtype=F32, device=dev)
    O.nchw_rows_f32(y, B, C, HW, cpad, back[64:], ld, to_rows=False)
    torch.cuda.synchronize()
    expb = torch.full_like(back, SENT)
    expb[64:64 + B * C * HW] = x.reshape(-1)
    assert R.same_bits(back, expb)


# ====================================================================== 4. pack table
def test_pack_weights_table(O, L):
    """One launch, 20 jobs, bitwise against restatements written from the header's layouts, gaps
    between destinations at the sentinel, two calls agree.  Catches: the vector path's last
    16-byte store or its stride loop's second pass (total 262,656 > 128 x 256 x 8) dropped; the
    scalar path taken for the wrong reason (total = 100, src_off = 2, dst_off = 4 each force it) or
    its second pass (total 32,771 > 32,768) dropped; tap / channel order of kinds 1-4 transposed;
    hi / lo blocks swapped; kind 5's identity transposed or shifted; kind 6 ragged tiles (70 x 45,
    1 x 129) writing past the matrix."""
    g = _gen(44)
    spec = [  # (rows, cols, kind, cin, src_misalign, dst_misalign)
        (513, 512, 0, 0, 0, 0), (1, 100, 0, 0, 0, 0), (4, 16, 0, 0, 2, 0), (4, 16, 0, 0, 0, 4),
        (1, 32771, 0, 0, 0, 0),
        (32, 144, 1, 16, 0, 0), (7, 45, 1, 5, 0, 0),
        (6, 72, 2, 3, 0, 0), (6, 128, 2, 3, 0, 0), (6, 72, 2, 8, 0, 0),
        (5, 3 * 24 * 16, 3, 24, 0, 0), (8, 3 * 16 * 9, 3, 16, 0, 0),
        (4, 24 * 16, 4, 3, 0, 0),
        (32, 160, 5, 32, 0, 0), (128, 640, 5, 128, 0, 0),
        (32, 32, 6, 0, 0, 0), (70, 45, 6, 0, 0, 0), (1, 129, 6, 0, 0, 0), (192, 64, 6, 0, 0, 0)]
    jobs, so, do = [], 0, 16
    for rows, cols, kind, cin, sm, dm in spec:
        so = (so + 3) // 4 * 4 + sm
        do = (do + 7) // 8 * 8 + dm
        jobs.append(L.PackJob(src_off=so, dst_off=do, rows=rows, cols=cols, kind=kind, cin=cin))
        so += R.pack_src_elems(rows, cols, kind, cin) + 3
        do += rows * cols + 11  # a gap of at least 11 sentinels after every job
    assert len(jobs) >= 10
    src = rnd(g, so + 8, scale=3.0, specials=True)
    exp = torch.full((do + 64,), SENT, dtype=BF16, device=dev)
    for j in jobs:
        exp[j.dst_off:j.dst_off + j.rows * j.cols] = R.pack_ref(src, j.src_off, j.rows, j.cols, j.kind, j.cin)
    jt = torch.frombuffer(bytearray((L.PackJob * len(jobs))(*jobs)), dtype=torch.uint8).to(dev)
    outs = []
    for _ in range(2):
        dst = torch.full_like(exp, SENT)
        O.pack_weights(src, dst, jt, len(jobs))
        torch.cuda.synchronize()
        outs.append(dst)
    for k, j in enumerate(jobs):
        a = outs[0][j.dst_off:j.dst_off + j.rows * j.cols]
        assert R.same_bits(a, exp[j.dst_off:j.dst_off + j.rows * j.cols]), f"job {k} kind {j.kind}"
    assert R.same_bits(outs[0], exp), "a gap between jobs was written"
    assert R.same_bits(outs[0], outs[1])


# ====================================================================== 5. AdamW + EMA + mirror
def _hyper(O, step, omd):
    return torch.tensor(O.adamw_hyper(1e-3, step, weight_decay=0.05, ema_one_minus_decay=omd), dtype=F32, device=dev)


@pytest.mark.parametrize("ema_mode", ["none", "all", "r1", "r2", "r3"])
@pytest.mark.parametrize("n", [4, 1028, 4194304 + 12])
def test_adamw_ema_mirror(O, n, ema_mode):
    """Three steps (bias corrections of steps 1, 2, 1000), weight decay 0.05, gradients with exact
    zeros and 1e-20, per element against torch.optim.AdamW + LitEma in fp64 on the state the kernel
    started the step from.  ema_n = n - 100 - r (4 - r at n = 4) ends inside a float4 lane: the
    lane's live elements must be updated and the elements at and past ema_n (inside the storage,
    rounded up to 4 floats) bitwise unchanged.  mirror == p.to(bfloat16); mirror = None leaves a
    sentinel buffer alone; the two-range form of DiffusionOptimizer.launch_part gives the single
    launch's bits.  Catches: EMA tail lane not updated or the dead lanes rewritten with new values,
    elements past 4096 x 256 x 4 skipped, mirror written from the pre-update weight, eps added
    before the bias correction, decay coupled into the gradient.
    Largest floors measured on the MI355X (4 x torch fp32 vs fp64): p 2.0e-6, m 2.0e-7, v 9.6e-9,
    ema 2.1e-6; the kernel's largest distances from fp64: p 2.8e-7, m 5.0e-8, v 2.4e-9, ema 4.3e-7."""
    g = _gen(n % 1000 + len(ema_mode))
    r = {"none": 0, "all": 0, "r1": 1, "r2": 2, "r3": 3}[ema_mode]
    ema_n = 0 if ema_mode == "none" else (n if ema_mode == "all" else (n - 100 - r if n > 104 else n - r))
    store_n = (ema_n + 3) // 4 * 4
    p = rnd(g, n)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ema_store = torch.full((store_n + 8,), SENT, device=dev)
    ema_store[:ema_n] = p[:ema_n] * 0.5
    ema = ema_store if ema_n else None
    mirror = torch.full((n + 8,), SENT, dtype=BF16, device=dev)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ema2 = ema_store.clone()
    mirror2 = mirror.clone()
    for step in (1, 2, 1000):
        gr = rnd(g, n)
        gr[::5] = 0.0
        gr[1::7] = 1e-20
        hy = _hyper(O, step, 1 - min(0.9999, (1 + step) / (10 + step)))
        s0 = (p.clone(), m.clone(), v.clone(), ema_store[:ema_n].clone() if ema_n else None)
        dead = ema_store[ema_n:].clone()
        O.adamw_ema(p, gr, m, v, hy, ema=ema, ema_n=ema_n, mirror=mirror)
        # the same step as two ranges split at ema_n rounded up to 4
        mid = store_n
        if mid > 0:
            O.adamw_ema(p2[:mid], gr[:mid], m2[:mid], v2[:mid], hy, ema=ema2 if ema_n else None, ema_n=ema_n,
                        mirror=mirror2[:mid])
        if n > mid:
            O.adamw_ema(p2[mid:], gr[mid:], m2[mid:], v2[mid:], hy, ema=None, ema_n=0, mirror=mirror2[mid:n])
        torch.cuda.synchronize()
        for a, b, nm in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v"), (ema_store, ema2, "ema"), (mirror, mirror2, "mirror")):
            assert R.same_bits(a, b), f"two-range {nm} differs at step {step}"
        assert R.same_bits(ema_store[ema_n:], dead), "EMA elements at / past ema_n changed"
        assert R.same_bits(mirror[:n], p.to(BF16)) and (mirror[n:] == SENT).all()
        r64 = R.adamw_ema_step(s0[0].double(), gr.double(), s0[1].double(), s0[2].double(),
                               None if s0[3] is None else s0[3].double(), ema_n, hy.double())
        r32 = R.adamw_ema_step(s0[0], gr, s0[1], s0[2], s0[3], ema_n, hy)
        for out, a64, a32, nm in ((p, r64[0], r32[0], "p"), (m, r64[1], r32[1], "m"), (v, r64[2], r32[2], "v")):
            assert_f32_rule(out, a64, a32, f"adamw n={n} {ema_mode} step {step} {nm}")
        if ema_n:
            assert_f32_rule(ema_store[:ema_n], r64[3], r32[3], f"adamw n={n} {ema_mode} step {step} ema")
    # mirror = None: nothing is written through a mirror pointer
    O.adamw_ema(p, gr, m, v, hy, ema=ema, ema_n=ema_n, mirror=None)
    torch.cuda.synchronize()
    assert R.same_bits(mirror[:n], p2.to(BF16)) and (mirror[n:] == SENT).all()


def test_arena_ema_storage_rounded(O):
    """ParamArena.enable_ema(): ema is the [:ema_numel] view of storage rounded up to a multiple of
    4 floats (the float4 lane the optimizer rewrites), so an ema_numel % 4 != 0 arena gives the
    kernel nothing outside its allocation.  Catches a return to the exact-size clone."""
    from encdiff_amd.arena import ParamArena
    ps = [("a", torch.nn.Parameter(torch.randn(8, 3))), ("b", torch.nn.Parameter(torch.randn(5))),
          ("c", torch.nn.Parameter(torch.randn(16)))]
    a = ParamArena(ps, dev, ema_names=["a", "b"])
    assert a.ema_numel == 29
    ema = a.enable_ema()
    assert ema.numel() == 29 and ema.untyped_storage().nbytes() >= 32 * 4 and ema.data_ptr() % 16 == 0
    assert torch.equal(ema, a.master[:29]) and torch.equal(a.view_in(ema, "b"), a.master[24:29])
    a.grad.normal_()
    before = a._ema_store.clone()
    hy = _hyper(O, 1, 0.25)
    O.adamw_ema(a.master, a.grad, a.exp_avg, a.exp_avg_sq, hy, ema=a.ema, ema_n=a.ema_numel, mirror=None)
    torch.cuda.synchronize()
    assert R.same_bits(a._ema_store[29:], before[29:])
    exp = before[:29].double() - 0.25 * (before[:29].double() - a.master[:29].double())
    assert (a.ema.double() - exp).abs().max() < 1e-6


# ====================================================================== 6. diffusion math
@pytest.fixture(scope="module")
def sched():
    from oracle import encdiff_oracle as OR
    return {k: v.to(dev) for k, v in OR.sched_fp32(OR.register_schedule()).items()}


@pytest.mark.parametrize("lsw", [1.0, 0.25])
@pytest.mark.parametrize("batch,per", [(1, 48), (3, 768), (257, 1000), (600, 768)])
def test_l1_loss(O, sched, batch, per, lsw):
    """L1 loss and its gradient seed, with and without `grad`, ~1% exact ties, t including 0 and
    999, called twice.  Losses within 2^-20 relative of fp64 (a sum of <= 1000 terms in 4-lane,
    wave and fixed-order stages: each stage's error <= log2-depth x 2^-24, 8 x margin); the gradient
    bitwise sign(pred - eps) * (lsw / (batch * per)); the ticket reads zero after every call.
    Catches: the fold loop skipping samples >= 256, a tail of per % 256 dropped, lsw applied to the
    loss but not the gradient, a tie given +-scale, a ticket left at `batch`, `grad = NULL` written."""
    g = _gen(batch + per)
    pred, eps = rnd(g, batch, per), rnd(g, batch, per)
    tie = torch.rand(batch, per, generator=g).to(dev) < 0.01
    pred[tie] = eps[tie]
    pred[0, per - 1] = eps[0, per - 1]
    t = torch.randint(0, 1000, (batch,), generator=g).to(dev)
    t[0] = 999
    t[-1] = 0 if batch > 1 else 999
    ref_loss, ref_vlb, ref_ls = R.l1_loss(pred, eps, t, sched["lvlb_weights"], lsw)
    tick = O.scratch("l1_ticket", 1, torch.int32, pred.device.index)
    outs = []
    for with_grad in (True, False, True):
        out2 = torch.full((2 + 6,), SENT, device=dev)
        grad = Guard(batch, per, F32)
        O.l1_loss(pred, eps, t, sched["lvlb_weights"], out2[:2], grad.view if with_grad else None, lsw)
        torch.cuda.synchronize()
        assert int(tick.item()) == 0
        assert (out2[2:] == SENT).all()
        grad.check()
        print(f"l1 {batch}x{per} lsw={lsw}: loss rel {abs(out2[0].item() / ref_loss.item() - 1):.2e} "
              f"vlb rel {abs(out2[1].item() / ref_vlb.item() - 1):.2e}")
        assert abs(out2[0].double().item() - ref_loss.item()) <= 2.0 ** -20 * abs(ref_loss.item())
        assert abs(out2[1].double().item() - ref_vlb.item()) <= 2.0 ** -20 * abs(ref_vlb.item())
        part = O.scratch("l1_partials", batch, F32, pred.device.index)[:batch]
        assert ((part.double() - ref_ls).abs() <= 2.0 ** -20 * ref_ls.abs()).all()
        if with_grad:
            assert R.same_bits(grad.view.contiguous(), R.l1_grad(pred, eps, lsw))
            assert (grad.view[tie] == 0).all()
            outs.append((out2.clone(), grad.view.clone()))
        else:
            assert (grad.view == SENT).all()
    assert R.same_bits(outs[0][0], outs[1][0]) and R.same_bits(outs[0][1], outs[1][1])


@pytest.mark.parametrize("scaled", [0, 1])
@pytest.mark.parametrize("B,per", [(1, 5), (1, 768), (16, 5), (16, 768), (14, 75000)])
def test_q_sample(O, sched, B, per, scaled):
    """q_sample and q_sample_scaled (scale a device scalar, 0.37) per element against fp64; t
    includes 0 and 999; 14 x 75000 = 1,050,000 elements is over the capped grid.  Catches: the
    scale applied to eps or to x_t, t indexed per element instead of per sample, the second pass of
    the stride loop dropped, the last (odd) element skipped.  Largest floor measured on the MI355X: 2.0e-6 (kernel 5.0e-7 from fp64)."""
    g = _gen(B * per + scaled)
    x0, eps = rnd(g, B, per, scale=2.0), rnd(g, B, per)
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    t[0] = 999
    t[-1] = 0 if B > 1 else 999
    sc = torch.tensor([0.37], device=dev) if scaled else None
    xt = Guard(B, per, F32)
    O.q_sample(x0, eps, t, sched["sqrt_alphas_cumprod"], sched["sqrt_one_minus_alphas_cumprod"], xt.view, x0_scale=sc)
    torch.cuda.synchronize()
    xt.check()
    a, s = sched["sqrt_alphas_cumprod"], sched["sqrt_one_minus_alphas_cumprod"]
    assert_f32_rule(xt.view, R.q_sample(x0, eps, t, a, s, sc, F64), R.q_sample(x0, eps, t, a, s, sc, F32),
                    f"q_sample {B}x{per} scaled={scaled}")


@pytest.fixture(scope="module")
def ddim_rows(sched):
    """(a_t, a_prev, sigma, sqrt(1 - a_t)) at the first, a middle and the last index of the eta = 0
    and eta = 1 tables at S = 50, as fp32."""
    from oracle import encdiff_oracle as OR
    rows = []
    for eta in (0.0, 1.0):
        d = OR.ddim_schedule(sched["alphas_cumprod"].cpu(), 50, eta)
        for i in (0, 25, 49):
            rows.append([float(torch.tensor(d[k][i], dtype=F32)) for k in
                         ("alphas", "alphas_prev", "sigmas", "sqrt_one_minus_alphas")])
    return rows


@pytest.mark.parametrize("n", [5, 1048576 + 5])
def test_ddim_step(O, ddim_rows, n):
    """DDIM update per element against fp64 for six coefficient rows, with `noise` and `pred_x0`
    each present and absent.  Catches: sigma z added when noise is NULL garbage, pred_x0 written
    through a NULL pointer's neighbour, sqrt(1 - a_prev - sigma^2) formed without sigma, elements
    past 4096 x 256 skipped, the 5-element tail dropped.  Largest floors measured on the
    MI355X: x_prev 6.5e-6, pred_x0 1.2e-4 (the last row's 1 / sqrt(a_t) amplifies the fp32 rounding
    of x - s1 e); the kernel's largest distances from fp64: 1.4e-6 and 2.5e-5."""
    g = _gen(n % 97)
    x, e, z = rnd(g, 1, n), rnd(g, 1, n), rnd(g, 1, n)
    for ri, (a_t, a_prev, sigma, s1) in enumerate(ddim_rows):
        for has_noise, has_px0 in ((1, 1), (0, 1), (1, 0)) if ri in (0, 5) else ((1, 1),):
            xp, px = Guard(1, n, F32), Guard(1, n, F32)
            O.ddim_step(x, e, z if has_noise else None, a_t, a_prev, sigma, s1, xp.view, px.view if has_px0 else None)
            torch.cuda.synchronize()
            xp.check()
            px.check()
            noise = z if has_noise else None
            r64 = R.ddim_step(x, e, noise, a_t, a_prev, sigma, s1, F64)
            r32 = R.ddim_step(x, e, noise, a_t, a_prev, sigma, s1, F32)
            what = f"ddim n={n} row {ri} noise={has_noise} px0={has_px0}"
            assert_f32_rule(xp.view, r64[0], r32[0], what + " x_prev")
            if has_px0:
                assert_f32_rule(px.view, r64[1], r32[1], what + " pred_x0")
            else:
                assert (px.view == SENT).all()


def test_ddim_step_indexed(O, ddim_rows):
    """The graph form reads its row from a device table: bitwise ddim_step with the same row;
    advance = 1 decrements the device index by exactly one per call (three calls, 3 -> 0),
    advance = 0 leaves it.  Catches: the row read at index * 3 or index + 1, a decrement before
    the read, a double decrement, the table's sigma and s1 columns exchanged."""
    n = 1048576 + 5
    g = _gen(5)
    x, e, z = rnd(g, 1, n), rnd(g, 1, n), rnd(g, 1, n)
    sel = [ddim_rows[3], ddim_rows[4], ddim_rows[5], ddim_rows[1]]
    coef = torch.tensor(sel, dtype=F32, device=dev)
    idx = torch.tensor([3], dtype=torch.int32, device=dev)
    for k in (3, 2, 1):
        xp, px, xr, pr = (Guard(1, n, F32) for _ in range(4))
        O.ddim_step_indexed(x, e, z, coef, idx, xp.view, px.view, advance=True)
        O.ddim_step(x, e, z, *sel[k], xr.view, pr.view)
        torch.cuda.synchronize()
        assert int(idx.item()) == k - 1
        xp.check()
        px.check()
        assert R.same_bits(xp.buf, xr.buf) and R.same_bits(px.buf, pr.buf)
    xp, xr = Guard(1, 5, F32), Guard(1, 5, F32)
    O.ddim_step_indexed(x[:, :5], e[:, :5], None, coef, idx, xp.view, None, advance=False)
    O.ddim_step(x[:, :5], e[:, :5], None, *sel[0], xr.view, None)
    torch.cuda.synchronize()
    assert int(idx.item()) == 0 and R.same_bits(xp.buf, xr.buf)


@pytest.mark.parametrize("batch", [1, 6, 300])
@pytest.mark.parametrize("dim", [64, 128, 256])
def test_timestep_embedding(O, dim, batch):
    """bf16 and fp32 timestep embeddings per element against fp64, t covering 0, 1, 2, 500, 998,
    999 (batch 1: one launch per value).  bf16: 2^-7 |ref| + 999 * 2^-20 (a frequency accurate to
    2^-20 relative: 8 x a correctly rounded fp32 value, room for the fast exponential).  fp32:
    4 x the host torch fp32 evaluation's distance + 2^-22 |ref|; measured floors 1.4e-4 (dim 64),
    2.1e-4 (dim 128), 2.2e-4 (dim 256), the kernel itself within 3.6e-5 / 5.3e-5 / 5.6e-5 of fp64.
    The bf16 kernel's largest distance from fp64 is 1.98e-3 at |ref| ~ 1 (half a bf16 ulp).  Catches: cos / sin halves exchanged, k / dim instead of
    k / half, t read as int32, rows past the first workgroup (300 x 128 threads) skipped."""
    tv = [0, 1, 2, 500, 998, 999]
    g = _gen(dim + batch)
    if batch == 1:
        ts = [torch.tensor([v]) for v in tv]
    else:
        t = torch.randint(0, 1000, (batch,), generator=g)
        t[:6] = torch.tensor(tv)
        ts = [t]
    for t in ts:
        td = t.to(dev)
        ref = R.timestep_embedding(t, dim).to(dev)
        t32 = R.timestep_embedding(t, dim, dtype=F32).to(dev)  # on the host, as the quoted figures
        ob, of = Guard(batch, dim, BF16), Guard(batch, dim, F32)
        O.timestep_embedding(td, dim, ob.view)
        O.timestep_embedding_f32(td, dim, of.view)
        torch.cuda.synchronize()
        ob.check()
        of.check()
        ex, i, worst = R.bf16_excess(ob.view, ref, 999 * 2.0 ** -20)
        print(f"temb bf16 dim={dim} batch={batch}: max|out-ref| {worst:.3e} excess {ex:.3e}")
        assert ex <= 0, f"bf16 embedding element {i}: over the bound by {ex:.3e}"
        assert_f32_rule(of.view, ref, t32, f"temb f32 dim={dim} batch={batch} t0={int(t[0])}")


# ====================================================================== 7. gradient plumbing
@pytest.mark.parametrize("rows", [1, 7, 8, 25, 33, 100])
def test_reduce_partials(O, rows):
    """Column sums of part[:rows, :cols] (ld > cols) added into a scattered permutation of a larger,
    nonzero gradient; cols in 1, 31, 33, 50.  Within 2^-20 x sum|part| per column of fp64 (at most
    100 fp32 adds, error <= 100 x 2^-24 x sum|part| / 2 on average, well inside), untouched
    entries bitwise, two calls bitwise.  Catches: the unrolled 4-row loop (rows > 24) skipping or
    double counting rows 8u + slice, the row tail dropped, column 32 of a 33-column job lost,
    `=` instead of `+=`, index read at column + 1."""
    for cols in (1, 31, 33, 50):
        g = _gen(rows * 64 + cols)
        ld = cols + 5
        part = rnd(g, rows + 2, ld, scale=2.0)
        idx = torch.randperm(200, generator=g)[:cols].to(torch.int32).to(dev)
        g0 = rnd(g, 200)
        ref, scale = R.reduce_partials_ref64(part, rows, cols)
        res = []
        for _ in range(2):
            gr = g0.clone()
            O.reduce_partials(part, ld, rows, cols, idx, gr)
            torch.cuda.synchronize()
            res.append(gr)
        got = res[0][idx.long()].double() - g0[idx.long()].double()
        # + the rounding of the stored fp32 sum grad + t (half an ulp of a nonzero target)
        tol = 2.0 ** -20 * scale + 2.0 ** -24 * (g0[idx.long()].double().abs() + ref.abs())
        assert ((got - ref).abs() <= tol).all(), f"rows {rows} cols {cols}"
        mask = torch.ones(200, dtype=torch.bool, device=dev)
        mask[idx.long()] = False
        assert R.same_bits(res[0][mask], g0[mask]) and R.same_bits(res[0], res[1])


@pytest.mark.parametrize("with_bias", [0, 1])
@pytest.mark.parametrize("co,cin,cpad,taps", [(64, 3, 8, 9), (3, 64, 64, 9), (128, 3, 8, 16), (256, 4, 8, 9)])
def test_grad_fold(O, co, cin, cpad, taps, with_bias):
    """gw[o][c][t] += dw[o][t][c] bitwise against gw + dw.permute, gb += db with db left exactly
    zero, gw / gb nonzero on entry, dw's padding channels at a sentinel that must not leak, two
    calls agree.  Catches: taps and channels exchanged, cpad taken for cin in the source stride, a
    padding channel folded in, db not cleared (double counted at the next replay), bias of
    channels >= 256 threads lost."""
    g = _gen(co + taps)
    dw = rnd(g, co * taps * cpad, scale=2.0)
    dw.view(co, taps, cpad)[:, :, cin:] = SENT
    gw0, gb0, db0 = rnd(g, co * cin * taps), rnd(g, co), rnd(g, co)
    exp_w = R.grad_fold_ref(gw0, dw, co, cin, cpad, taps).reshape(-1)
    res = []
    for _ in range(2):
        gw = torch.full((co * cin * taps + 16,), SENT, device=dev)
        gw[:co * cin * taps] = gw0
        gb, db = gb0.clone(), db0.clone()
        O.grad_fold(dw, co, cin, cpad, taps, gw[:co * cin * taps], db if with_bias else None, gb if with_bias else None)
        torch.cuda.synchronize()
        assert R.same_bits(gw[:co * cin * taps], exp_w) and (gw[co * cin * taps:] == SENT).all()
        if with_bias:
            assert R.same_bits(gb, gb0 + db0) and R.same_bits(db, torch.zeros_like(db))
        else:
            assert R.same_bits(gb, gb0) and R.same_bits(db, db0)
        res.append(gw)
    assert R.same_bits(res[0], res[1])


def test_grad_fold_rejects(O, L):
    """co = 257 (the bias fold is one 256-thread workgroup) and cin > cpad are refused before launch."""
    dw = torch.zeros(257 * 9 * 8, device=dev)
    with pytest.raises(L.HipError):
        O.grad_fold(dw, 257, 3, 8, 9, torch.zeros(257 * 3 * 9, device=dev))
    with pytest.raises(L.HipError):
        O.grad_fold(dw, 4, 9, 8, 9, torch.zeros(4 * 9 * 9, device=dev))


# ====================================================================== 8. input path, BatchNorm forms
@pytest.mark.parametrize("n,h,w,c", [(5, 2, 2, 3), (7, 6, 6, 3), (4, 6, 6, 1), (5, 8, 8, 1)])
def test_gather_images_u8_small(O, n, h, w, c):
    """Gather + ToTensor / Normalize / CHW == oracle.images_to_input bitwise on images whose byte
    size is not a multiple of 16 (byte-wise staging; image 1 of (7, 6, 6, 3) starts at byte 108)
    and on 64-byte images (16-byte staging); ids -1 and n are clamped to images 0 and n - 1 (the
    documented bounds guard); the device step selects the batch and advances by one.  Catches: the
    byte path's tail (nbytes % 256) dropped, HWC read as CHW, the clamp off by one, the step not
    applied to the perm offset."""
    from oracle import encdiff_oracle as OR
    g = _gen(n * h + c)
    pool = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)
    pool[0, 0, 0, 0], pool[-1, -1, -1, -1] = 0, 255
    batch = 6
    perm = torch.cat([torch.tensor([-1, n, 0, n - 1, 1, 2 % n]), torch.randint(0, n, (batch,), generator=g)])
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    for s in range(2):
        buf = torch.full((16 + batch * c * h * w + 16,), SENT, device=dev)
        out = buf[16:16 + batch * c * h * w].view(batch, c, h, w)
        O.gather_images_u8(pool.to(dev), perm.to(dev), step, batch, out, advance=True)
        torch.cuda.synchronize()
        ids = perm[s * batch:(s + 1) * batch].clamp(0, n - 1)
        exp = torch.full_like(buf, SENT)
        exp[16:16 + batch * c * h * w] = OR.images_to_input(pool, ids).reshape(-1).to(dev)
        assert R.same_bits(buf, exp)
        assert int(step.item()) == s + 1


def _bn_args(L, rows, C, relu, x, y, ldy, mean, rstd, gamma, beta, part, cnt, x_f32, y_split):
    return L.BatchNormArgs(rows=rows, c=C, eps=1e-5, momentum=0.1, relu=int(relu), x_f32=int(x_f32), x=x.data_ptr(),
                           ldx=x.stride(0), gamma=gamma.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(), ldy=ldy,
                           mean=mean.data_ptr(), rstd=rstd.data_ptr(), partials=part.data_ptr(),
                           counter=cnt.data_ptr(), y_split=int(y_split))


@pytest.mark.parametrize("rows", [50, 4099])
@pytest.mark.parametrize("C", [8, 32, 128, 256])
def test_batchnorm_forms(O, L, C, rows):
    """BatchNorm's untested forms against nn.BatchNorm2d restated in fp64, with and without ReLU:
    training forward on fp32 x (x_f32 = 1); y_split = 1 blocks [hi | lo | hi]; and
    encdiff_batchnorm_apply with the caller's mean / rstd.  bf16 outputs follow the bf16 rule; for
    y_split the third block equals the first bitwise and float(hi) + float(lo) is within
    2^-15 |ref| + floor.  Catches: fp32 x read with the bf16 row stride, lo written to block 2 and
    hi to block 1, lo = bf16(z) - hi (rounded first: zero), the apply form normalising with batch
    statistics, ReLU applied before the affine, the last of 4099 rows dropped.
    Largest floors measured on the MI355X: x_f32 forward 5.6e-6, y_split 4.9e-6, apply 6.7e-6;
    hi + lo is within 3.1e-5 of fp64 where the bound is 2^-15 |ref| + floor."""
    g = _gen(C + rows)
    x32 = rnd(g, rows, C, scale=2.0) + 0.5
    xb = x32.to(BF16)
    gamma, beta = torch.rand(C, generator=g).to(dev) + 0.5, rnd(g, C, scale=0.2)
    part = torch.empty(L.lib.encdiff_batchnorm_partials_floats(rows, C), device=dev)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    cmean, crstd = rnd(g, C, scale=0.3) + 0.5, torch.rand(C, generator=g).to(dev) + 0.3
    for relu in (0, 1):
        # training forward, fp32 input
        mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
        y = Guard(rows, C, BF16, strided=True)
        a = _bn_args(L, rows, C, relu, x32, y.view, y.view.stride(0), mean, rstd, gamma, beta, part, cnt, 1, 0)
        L.check(L.lib.encdiff_batchnorm_fwd(ctypes.byref(a), _stream()), "bn fwd x_f32")
        torch.cuda.synchronize()
        y.check()
        assert int(cnt.item()) == 0
        ref = R.batchnorm_train(x32, gamma, beta, 1e-5, relu, F64)[0]
        t32 = R.batchnorm_train(x32, gamma, beta, 1e-5, relu, F32)[0]
        assert_bf16_rule(y.view, ref, t32, f"bn x_f32 C={C} rows={rows} relu={relu}")
        # training forward, split output
        ys = Guard(rows, 3 * C, BF16, strided=True)
        a = _bn_args(L, rows, C, relu, xb, ys.view, ys.view.stride(0), mean, rstd, gamma, beta, part, cnt, 0, 1)
        L.check(L.lib.encdiff_batchnorm_fwd(ctypes.byref(a), _stream()), "bn fwd y_split")
        torch.cuda.synchronize()
        ys.check()
        ref = R.batchnorm_train(xb, gamma, beta, 1e-5, relu, F64)[0]
        t32 = R.batchnorm_train(xb, gamma, beta, 1e-5, relu, F32)[0]
        hi, lo, hi2 = ys.view[:, :C], ys.view[:, C:2 * C], ys.view[:, 2 * C:]
        assert R.same_bits(hi.contiguous(), hi2.contiguous())
        assert_bf16_rule(hi, ref, t32, f"bn y_split hi C={C} rows={rows} relu={relu}")
        floor = R.floor_of(t32, ref)
        err = (hi.double() + lo.double() - ref).abs()
        print(f"bn y_split hi+lo C={C} rows={rows} relu={relu}: floor {floor:.3e} max err {err.max().item():.3e}")
        assert (err <= 2.0 ** -15 * ref.abs() + floor).all()
        # eval form: the caller's statistics, plain and split
        for split in (0, 1):
            ya = Guard(rows, 3 * C if split else C, BF16, strided=True)
            a = _bn_args(L, rows, C, relu, xb, ya.view, ya.view.stride(0), cmean, crstd, gamma, beta, part, cnt, 0, split)
            L.check(L.lib.encdiff_batchnorm_apply(ctypes.byref(a), _stream()), "bn apply")
            torch.cuda.synchronize()
            ya.check()
            ref = R.batchnorm_apply(xb, cmean, crstd, gamma, beta, relu, F64)
            t32 = R.batchnorm_apply(xb, cmean, crstd, gamma, beta, relu, F32)
            assert_bf16_rule(ya.view[:, :C], ref, t32, f"bn apply C={C} rows={rows} relu={relu} split={split}")
            if split:
                assert R.same_bits(ya.view[:, :C].contiguous(), ya.view[:, 2 * C:].contiguous())
                err = (ya.view[:, :C].double() + ya.view[:, C:2 * C].double() - ref).abs()
                assert (err <= 2.0 ** -15 * ref.abs() + R.floor_of(t32, ref)).all()
