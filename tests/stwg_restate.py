"""Restatement of the grouped weight gradients of a fused transformer block (encdiff_st_wgrad_*,
csrc/st_bwd.hip and csrc/stwg.h), dtype- and device-generic torch:

  dW [M][N] = dW0 + dY^T X,   db [M] = db0 + column sums of dY,   dY [K][M], X [K][N] over K tokens.

`wgrad` is the plain statement.  `wgrad_chunked` follows the plan's order: the tokens are cut into
chunks of kc; a problem of one chunk is added straight onto dW0; otherwise every chunk z gives a
slab dY[z]^T X[z] (and a bias row), and the fold sums them in eight groups -- group g takes
z = g, g + 8, ... in order, starting from 0 -- then adds the groups in order 0..7 and the total
onto dW0.  On small integers both give the same bits; on rounded inputs the chunked one evaluated
in fp32 is the kernel's own summation order down to the chunk.
tests/test_stwg_restate.py checks both on the CPU; tests/test_gpu_st_wgrad.py compares the kernels.
"""
import torch


def wgrad(dy, x, dw0, db0, dt):
    dy, x = dy.to(dt), x.to(dt)
    return dw0.to(dt) + dy.t() @ x, (None if db0 is None else db0.to(dt) + dy.sum(0))


def chunks(K, kc):
    """Token spans [k0, k1) of the plan's chunks."""
    return [(k0, min(K, k0 + kc)) for k0 in range(0, K, kc)]


def slabs(dy, x, spans, dt):
    """Per chunk: (dY[z]^T X[z], column sums of dY[z])."""
    dy, x = dy.to(dt), x.to(dt)
    return [dy[a:b].t() @ x[a:b] for a, b in spans], [dy[a:b].sum(0) for a, b in spans]


def fold(parts):
    """stwg_fold_block's order: eight group sums over z = g, g + 8, ..., then the groups in order."""
    groups = []
    for g in range(8):
        a = torch.zeros_like(parts[0])
        for z in range(g, len(parts), 8):
            a = a + parts[z]
        groups.append(a)
    t = groups[0]
    for k in range(1, 8):
        t = t + groups[k]
    return t


def wgrad_chunked(dy, x, dw0, db0, kc, dt):
    spans = chunks(dy.shape[0], kc)
    if len(spans) == 1:  # accumulated in place, no slab and no fold
        return wgrad(dy, x, dw0, db0, dt)
    ws, bs = slabs(dy, x, spans, dt)
    return dw0.to(dt) + fold(ws), (None if db0 is None else db0.to(dt) + fold(bs))
