"""What every captured sampling loop is built from: the side-stream graph capture, the scope of
the UNet inside a loop (eps borrow, hoisted K / V and FiLM rows), one noise source of a loop
(NoiseRows), the whole-loop / one-step path policy, and the input rules the captured and the eager
loops share (kernel_mask, noise_table, vq_codebook).  The loops themselves -- DDIM sampling and
inversion in ldm/models/diffusion/ddim.py, the ancestral step in ddpm_enc.py, the VQ decode in
vq.py -- keep their own buffers and node order."""
from __future__ import annotations

from contextlib import contextmanager

import torch

from . import ops


def capture(body, restore=None, warm=False):
    """``body()`` captured on a side stream into a new torch.cuda.CUDAGraph.  warm: one eager
    ``body()`` first (allocations, kernel attributes, GEMM plans happen outside the capture).
    restore: a tensor the body updates in place; it is cloned first and copied back after the
    warm-up and after the capture, so the first replay starts from the caller's value."""
    keep = None if restore is None else restore.clone()
    if warm:
        body()
        if keep is not None:
            restore.copy_(keep)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            body()
    torch.cuda.current_stream().wait_stream(s)
    if keep is not None:
        restore.copy_(keep)
    return g


@contextmanager
def unet_loop(ldm, ts_col=None):
    """The UNet of ``ldm`` inside a sampling loop.  The HIP UNet hands its eps buffer over without
    a copy (borrow_eps): each loop step consumes e_t before the next forward overwrites it.
    ts_col, the loop's timesteps (S,), on the bf16 executor: the conditioning is fixed and every row
    shares t within the loop, so the executor computes the concept-token K / V once and the FiLM rows
    of all S steps in one pass at step 0 (UNetExecutor.samp_ts / samp_i).  Yields ``at(i)``, to be
    called in front of step i's forward.  Both are undone on the way out, also when the body raises."""
    um = getattr(getattr(ldm, "model", None), "diffusion_model", None)
    hip = um is not None and hasattr(um, "executor")
    ex = None
    if hip and ts_col is not None and getattr(um, "hip_precision", "bf16") != "fp32":
        ex = um.executor()
        ex.samp_ts, ex.samp_i = ts_col, None
    if hip:
        um.borrow_eps = True

    def at(i):
        if ex is not None:
            ex.samp_i = i

    try:
        yield at
    finally:
        if ex is not None:
            ex.samp_ts = ex.samp_i = None
        if hip:
            um.borrow_eps = False


class NoiseRows:
    """One N(0, I) source of a captured loop of ``total`` steps.  injected: a caller's table of
    ``total`` draws, copied in by fill() before a replay; else one row, drawn in place inside the
    graph on every read (draw=False: never drawn, the zeros of a loop whose sigma is 0)."""

    def __init__(self, total, shape, device, injected, draw=True):
        self.injected = bool(injected)
        self.draw = bool(draw) and not self.injected
        self.table = torch.zeros((total if self.injected else 1), *shape, device=device)
        self.indexed = self.table.shape[0] > 1  # rows are looked up by loop step
        self._buf = None  # row_at's row: a graph cannot index by a host value that changes per replay

    def fill(self, seq):
        if self.injected:
            self.table.copy_(seq[:self.table.shape[0]])

    def row(self, i):
        """The row of loop step i, i known on the host (unrolled loops)."""
        if self.draw:
            self.table[0].normal_()
        return self.table[i if self.indexed else 0]

    def row_at(self, counter):
        """The row of the loop step held by the device tensor ``counter`` (1,) int64 (one-step graphs)."""
        if not self.indexed:
            return self.row(0)
        if self._buf is None:
            self._buf = torch.empty_like(self.table[0])
        self._buf.copy_(self.table.index_select(0, counter).view_as(self._buf))
        return self._buf


def loop_or_step(seen, key, total, loop_after, max_steps):
    """Which captured path a call of the loop ``key`` takes.  Capturing a whole S-step loop only
    pays when the same loop is run again: its first ``loop_after`` calls replay the one-step graph,
    later ones the whole-loop graph.  Loops of more than ``max_steps`` steps always replay the
    one-step graph and are not counted in ``seen``."""
    if total > max_steps:
        return "step"
    n = seen.get(key, 0)
    seen[key] = n + 1
    return "loop" if n >= loop_after else "step"


def noise_table(seq, total, shape, device, what="normals_sequence"):
    t = torch.stack(list(seq)) if not isinstance(seq, torch.Tensor) else seq
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.shape[0] < total or tuple(t.shape[1:]) != tuple(shape):
        raise ValueError(f"{what} must hold {total} draws of shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def kernel_mask(mask, img):
    """mask as fp32 (B, 1, H, W) or (B, C, H, W) on img's device; None: another broadcast shape
    (the torch expression of the eager loop handles it)."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 4:
        return None
    B, C, H, W = img.shape
    if tuple(mask.shape) not in ((B, 1, H, W), (B, C, H, W)):
        return None
    return mask.to(device=img.device, dtype=torch.float32).contiguous()


def vq_codebook(ldm, img):
    """The first stage's codebook [n_e][e_dim] when the quantised-x0 kernels cover it (a VQ
    first stage, e_dim == the latent's channels, within the kernels' limits), else None."""
    q = getattr(getattr(ldm, "first_stage_model", None), "quantize", None)
    w = getattr(getattr(q, "embedding", None), "weight", None)
    if w is None or not img.is_cuda or w.dim() != 2 or w.shape[1] != img.shape[1]:
        return None
    if not ops.vq_supported(w.shape[0], w.shape[1]) or w.dtype != torch.float32 or not w.is_contiguous():
        return None
    return w.detach()
