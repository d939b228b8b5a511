"""Per-element tests of step_prologue_kernel (csrc/elementwise.hip, ops.StepPrologue) on the MI355X
against tests/prologue_restate.py: the timesteps bit for bit, the noise per element against the
fp64 evaluation of the Box-Muller formula on the same float32 uniforms, and every zero job byte for
byte inside non-zero sentinel `Guard`s.

Kernel branch -> test
  philox10: key = (seed lo, seed hi), counter (i, ctr lo, ctr hi, stream),
    round structure, multipliers, key schedule ......................... test_t_bitwise, test_noise
  t: (r.x * timesteps) >> 32, timesteps 1000 / 1, grid-stride second lap
    (batch 16,400 > 64 x 256) .......................................... test_t_bitwise
  noise: n_noise % 4 = 1 / 2 / 3 tails, one quad, 98,304 (training shape),
    second lap of the 64-workgroup grid + 3-element tail (65,539), second
    lap of the 2048-workgroup grid (2,097,155 with a zero job) ......... test_noise
  t NULL / noise NULL / both, data_step NULL / present, the ticket that
    advances the counters and resets `done` ............................ test_independence
  zero jobs: flat sweep (contiguous rows, one row of a strided tensor,
    one vector), its second lap (8 MiB + 48 B), strided rows (bf16 column
    slice), the 32-bit row / column split with 129 vectors per row and
    its second lap (528,900 vectors) ................................... test_zero_jobs
"""
import pytest
import torch

import elementwise_restate as R
import prologue_restate as P
from test_gpu_elementwise import Guard, assert_f32_rule

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
SEEDS = [0, 1234, 0xFFFFFFFF00000001]
COUNTERS = [0, 7, (1 << 32) - 1, (1 << 32) + 5]


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from encdiff_amd import ops
    return ops


def _pro(O, seed, counter):
    pro = O.StepPrologue(dev, seed)
    pro.counter.fill_(counter)
    return pro


def _after(pro, counter):
    """The launch advanced the counter by one and left the ticket at 0."""
    assert pro.counter.item() == counter + 1 and pro.done.item() == 0


def _flat(guard):
    return guard.view.view(-1)  # a one-row Guard: contiguous


def _check_t(guard, seed, counter, batch, timesteps):
    guard.check()
    want = torch.from_numpy(P.draw_t(seed, counter, batch, timesteps)).to(dev)
    got = _flat(guard)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"t seed={seed:#x} counter={counter} T={timesteps}: {bad.numel()} of {batch} differ, "
                              f"first b={int(bad[0])}: got {got[int(bad[0])].item()} want {want[int(bad[0])].item()}")


def _check_noise(guard, seed, counter, n, what):
    guard.check()
    u = torch.from_numpy(P.draw_u(seed, counter, n)).to(dev)
    assert_f32_rule(_flat(guard), P.box_muller(u, F64)[:n], P.box_muller(u, F32)[:n], what)


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_t_bitwise(O, seed, counter):
    """t[b] for batch 1 / 257 / 16,400 (64 workgroups x 256 threads without zero jobs: a second
    lap) and timesteps 1000 / 1, bit for bit.  Seed 0xFFFFFFFF00000001 has a non-zero high key word,
    counters 2^32 - 1 and 2^32 + 5 exercise the carry into and the use of the high counter word.
    Catches: a wrong round constant or key bump, the key words or the two counter words exchanged,
    the high word dropped, t drawn from the noise stream (word 3 = 0), r.y used for r.x, a signed
    product, the second lap skipped; the Guard catches a write past t[batch - 1]."""
    for timesteps in (1000, 1):
        for batch in (1, 257, 16400):
            pro = _pro(O, seed, counter)
            t = Guard(1, batch, I64)
            pro(t=_flat(t), timesteps=timesteps)
            torch.cuda.synchronize()
            _check_t(t, seed, counter, batch, timesteps)
            _after(pro, counter)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 98304, 65539, 2097155])
def test_noise(O, n):
    """noise[0 .. n) per element: |out - ref64| <= floor + 2^-22 |ref64|, ref64 the fp64 Box-Muller
    value of the restatement's float32 uniforms, floor = 4 x max |torch fp32 evaluation - fp64|
    (measured on the device and printed; the fp32 evaluation rounds the angle pi * 2u, which the
    kernel's sincospif does not, so the floor is a few 1e-6).  n % 4 != 0 leaves a partial quad whose
    remaining elements must stay sentinels (the Guard).  65,539 without zero jobs: 16,385 quads on
    16,384 threads; 2,097,155 with one zero job registered: 524,289 quads on 2048 x 256 threads.
    Every seed / counter pair of the t test at n = 1023, one pair elsewhere.
    Catches: what test_t_bitwise catches, on the noise stream; cos and sin or the two pairs
    exchanged, u01 without the + 1 (log 0), a tail quad dropped or written whole.
    Measured on the MI355X, floor / worst |out - ref|: n <= 5: 9.7e-7 .. 1.8e-6 / 1.2e-7; n = 1023
    (twelve seed / counter pairs): 3.0e-6 .. 4.4e-6 / 2.8e-7 .. 4.2e-7; 98,304: 5.6e-6 / 4.3e-7;
    65,539: 5.2e-6 / 4.2e-7; 2,097,155: 6.4e-6 / 6.3e-7.  The rule needed no widening for the
    device's logf / sincospif: the kernel is about ten times closer to fp64 than the floor."""
    pairs = [(s, c) for s in SEEDS for c in COUNTERS] if n == 1023 else [(1234, (1 << 32) + 5)]
    for seed, counter in pairs:
        pro = _pro(O, seed, counter)
        scratch = None
        if n == 2097155:
            scratch = torch.ones(64, device=dev)
            pro.set_jobs([scratch])
        z = Guard(1, n, F32)
        pro(noise=_flat(z))
        torch.cuda.synchronize()
        _check_noise(z, seed, counter, n, f"noise n={n} seed={seed:#x} counter={counter}")
        _after(pro, counter)
        if scratch is not None:
            assert (scratch == 0).all()


def test_independence(O):
    """The t draw alone (noise NULL) and the noise draw alone (t NULL) give the joint draw's values;
    data_step advances by one when present and the launch works without it; a launch with neither
    still advances the counter.  `counter` + 1 and `done` = 0 after every launch, and consecutive
    launches of one object walk the counter: the second equals a fresh draw at counter + 1."""
    seed, counter, batch, n = 1234, (1 << 32) - 1, 257, 1023
    runs = {}
    for name, use_t, use_z, use_step in (("joint", 1, 1, 1), ("t", 1, 0, 0), ("z", 0, 1, 1), ("none", 0, 0, 0)):
        pro = _pro(O, seed, counter)
        t, z = Guard(1, batch, I64), Guard(1, n, F32)
        step = torch.full((1,), 41, dtype=I64, device=dev)
        pro(t=_flat(t) if use_t else None, noise=_flat(z) if use_z else None, data_step=step if use_step else None)
        torch.cuda.synchronize()
        t.check()
        z.check()
        _after(pro, counter)
        assert step.item() == 41 + use_step
        for g, used in ((t, use_t), (z, use_z)):
            if not used:
                assert R.same_bits(g.buf, g.before), name
        runs[name] = (_flat(t).clone(), _flat(z).clone())
    want_t = torch.from_numpy(P.draw_t(seed, counter, batch, 1000)).to(dev)
    assert torch.equal(runs["joint"][0], want_t)
    assert R.same_bits(runs["t"][0], runs["joint"][0]) and R.same_bits(runs["z"][1], runs["joint"][1])
    # two launches of one object: the second is the draw at counter + 1 (here the carry into the high word)
    pro = _pro(O, seed, counter)
    t = Guard(1, batch, I64)
    pro(t=_flat(t))
    pro(t=_flat(t))
    torch.cuda.synchronize()
    _check_t(t, seed, counter + 1, batch, 1000)
    assert pro.counter.item() == counter + 2 and pro.done.item() == 0


def _zero_regions():
    """(guard, region view) of the six jobs; every region is 16-byte aligned inside its Guard."""
    a = Guard(3, 1000, F32)                        # contiguous rows: one flat sweep of 750 vectors
    b = Guard(16, 64, BF16, ld=192, left=64)       # a bf16 column slice: strided rows of 8 vectors
    c = Guard(5, 96, F32, ld=128, left=16)         # one row of a strided tensor: rows == 1, flat
    d = Guard(1, 2097164, F32)                     # 8 MiB + 48 B: 524,291 vectors, the flat sweep's second lap
    e = Guard(4100, 516, F32, ld=524, left=4)      # 2064-B rows at stride 2096 B: 129 vectors a row, 528,900 in all
    f = Guard(1, 4, F32)                           # a single vector
    return [(a, a.view), (b, b.view), (c, c.view[2:3]), (d, _flat(d)), (e, e.view), (f, _flat(f))]


def _check_zeroed(guard, region, what):
    want = guard.before.clone()
    want.as_strided(region.size(), region.stride(), region.storage_offset()).zero_()
    bad = (R.bits(guard.buf) != R.bits(want)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements wrong, first at buffer index {int(bad[0])}"


def test_zero_jobs(O):
    """Six zero jobs in one launch, each inside a Guard full of non-zero sentinels and compared byte
    for byte with the buffer in which exactly the region is zero: first with t and noise drawn in
    the same launch (and checked), then with both NULL.  Catches: the last vector of a row or of the
    sweep dropped, a strided job swept flat (the gaps zeroed), the row / column split wrong when the
    vectors per row are not a power of two (129), vectors past 2048 x 256 skipped, a job of the
    table skipped or taken twice at another's address."""
    seed, counter = 1234, 7
    for draw in (True, False):
        regs = _zero_regions()
        pro = _pro(O, seed, counter)
        pro.set_jobs([r for _, r in regs])
        assert pro.njobs == 6
        t, z = Guard(1, 257, I64), Guard(1, 1023, F32)
        pro(t=_flat(t) if draw else None, noise=_flat(z) if draw else None)
        torch.cuda.synchronize()
        for i, (g, r) in enumerate(regs):
            _check_zeroed(g, r, f"zero job {i} draw={int(draw)}")
        if draw:
            _check_t(t, seed, counter, 257, 1000)
            _check_noise(z, seed, counter, 1023, "noise beside six zero jobs")
        else:
            assert R.same_bits(t.buf, t.before) and R.same_bits(z.buf, z.before)
        _after(pro, counter)
