"""CPU tests of tests/prologue_restate.py, the reference of tests/test_gpu_step_prologue.py: the
generator is Philox4x32-10 (the three known-answer vectors of the Random123 distribution), and the
counter layout, the timestep scaling, u01 and the Box-Muller evaluation are what the module says."""
import numpy as np
import pytest
import torch

import prologue_restate as P

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, out):
    got = P.philox4x32_10(np.array([ctr], dtype=np.uint64), key)
    assert got.dtype == np.uint32 and tuple(int(v) for v in got[0]) == out


def test_philox_is_vectorised_consistently():
    """A batch of counters gives the rows the single calls give."""
    ctrs = np.array([k[0] for k in KAT] + [(5, 7, 0, 1)], dtype=np.uint64)
    key = (0xA4093822, 0x299F31D0)
    rows = P.philox4x32_10(ctrs, key)
    for i in range(len(ctrs)):
        assert (rows[i] == P.philox4x32_10(ctrs[i:i + 1], key)[0]).all()


def _philox_ints(c, k):
    """The same rounds on Python integers (no numpy), for one counter."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("seed,counter", [(0, 0), (1234, 7), (0xFFFFFFFF00000001, (1 << 32) + 5), (5, (1 << 32) - 1)])
def test_counter_and_key_layout(seed, counter):
    """t uses (b, ctr_lo, ctr_hi, 1), noise (q, ctr_lo, ctr_hi, 0); the key is (seed lo, seed hi)."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    lo, hi = counter & 0xFFFFFFFF, counter >> 32
    t = P.draw_t(seed, counter, 300, 1000)
    assert t.dtype == np.int64 and t.min() >= 0 and t.max() < 1000
    for b in (0, 1, 299):
        assert int(t[b]) == (_philox_ints((b, lo, hi, 1), key)[0] * 1000) >> 32
    assert (P.draw_t(seed, counter, 300, 1) == 0).all()
    u = P.draw_u(seed, counter, 1023)
    assert u.shape == (256, 4) and u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    for q in (0, 255):
        r = _philox_ints((q, lo, hi, 0), key)
        want = [np.float32((np.float32(v) + np.float32(1.0)) * np.float32(2.0 ** -32)) for v in r]
        assert [float(v) for v in u[q]] == [float(v) for v in want]
    # a prefix of a longer draw: element i does not depend on n
    assert (P.draw_u(seed, counter, 5)[:2] == u[:2]).all()
    # the streams differ between steps and between t and noise
    assert (P.draw_t(seed, counter + 1, 300, 1000) != t).any()


def test_u01_rounds_in_float32():
    x = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFF7F, 0x01000003], dtype=np.uint32)
    u = P.u01(x)
    assert u.dtype == np.float32
    assert float(u[0]) == 2.0 ** -32 and float(u[1]) == 2.0 ** -31 and float(u[2]) == 1.0
    assert float(u[3]) == 1.0 - 2.0 ** -24  # 2^32 - 129 + 1 rounds down to 2^32 - 256
    assert float(u[4]) == (2.0 ** 24 + 4) * 2.0 ** -32  # 2^24 + 3 ties to the even 2^24 + 4; + 1 ties back to it


def test_box_muller_formula_and_moments():
    u = torch.from_numpy(P.draw_u(99, 3, 1 << 18))
    z64, z32 = P.box_muller(u, torch.float64), P.box_muller(u, torch.float32)
    assert z64.shape == (1 << 18,) and z32.dtype == torch.float32
    assert (z32.double() - z64).abs().max() < 2e-5
    q = u[7].double()
    m0, m1 = (-2 * q[0].log()).sqrt(), (-2 * q[2].log()).sqrt()
    want = torch.stack([m0 * torch.cos(2 * torch.pi * q[1]), m0 * torch.sin(2 * torch.pi * q[1]),
                        m1 * torch.cos(2 * torch.pi * q[3]), m1 * torch.sin(2 * torch.pi * q[3])])
    assert torch.allclose(z64[28:32], want, rtol=0, atol=1e-14)
    assert abs(z64.mean().item()) < 0.01 and abs(z64.std().item() - 1) < 0.01
    assert abs((z64 ** 4).mean().item() - 3) < 0.1
