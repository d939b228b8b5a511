"""Restatement of step_prologue_kernel's random draws (csrc/elementwise.hip), in numpy integers for
the generator and dtype-generic torch for the Box-Muller formula.

  Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1); a round maps the
  counter to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) with M0 = 0xD2511F53,
  M1 = 0xCD9E8D57 and then bumps the key by (0x9E3779B9, 0xBB67AE85); ten rounds.
  key = (low, high) word of the 64-bit seed.
  noise quad q:  counter (q, ctr_lo, ctr_hi, 0);   timestep b:  counter (b, ctr_lo, ctr_hi, 1)
  t[b] = (r0 * timesteps) >> 32
  u01(x) = (float32(x) + 1f) * 2^-32, both roundings in float32: (0, 1]
  noise[4q .. 4q + 3] = (m0 cos a0, m0 sin a0, m1 cos a1, m1 sin a1),
      m0 = sqrt(-2 ln u01(r0)), a0 = pi * 2 u01(r1), m1 = sqrt(-2 ln u01(r2)), a1 = pi * 2 u01(r3)

tests/test_prologue_restate.py checks the generator against the Random123 known-answer vectors;
tests/test_gpu_step_prologue.py compares the kernel with it.
"""
import math

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: [n][4] integers < 2^32, key: (k0, k1).  Returns [n][4] uint32."""
    c = [np.asarray(ctr, dtype=np.uint64)[:, i] & MASK for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def _counters(n, counter, stream):
    counter = int(counter) & ((1 << 64) - 1)
    c = np.empty((n, 4), dtype=np.uint64)
    c[:, 0] = np.arange(n, dtype=np.uint64) & MASK
    c[:, 1] = counter & 0xFFFFFFFF
    c[:, 2] = counter >> 32
    c[:, 3] = stream
    return c


def _key(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def draw_t(seed, counter, batch, timesteps):
    """The batch's timesteps, int64 [batch]."""
    r = philox4x32_10(_counters(batch, counter, 1), _key(seed))
    return ((r[:, 0].astype(np.uint64) * np.uint64(timesteps)) >> np.uint64(32)).astype(np.int64)


def u01(x):
    """uint32 -> float32 in (0, 1]; conversion and addition round to nearest even in float32."""
    return (x.astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -32)


def draw_u(seed, counter, n_noise):
    """The uniforms behind noise[0 .. n_noise): float32 [ceil(n_noise / 4)][4]."""
    nq = (n_noise + 3) // 4
    return u01(philox4x32_10(_counters(nq, counter, 0), _key(seed)))


def box_muller(u, dt):
    """u: torch float32 [nq][4] -> the 4 nq normal values in dtype dt, evaluated in dt."""
    u = u.to(dt)
    m0, m1 = torch.sqrt(-2.0 * torch.log(u[:, 0])), torch.sqrt(-2.0 * torch.log(u[:, 2]))
    a0, a1 = math.pi * (2.0 * u[:, 1]), math.pi * (2.0 * u[:, 3])
    return torch.stack([m0 * torch.cos(a0), m0 * torch.sin(a0), m1 * torch.cos(a1), m1 * torch.sin(a1)], 1).reshape(-1)
