"""Pure-torch restatement of the 3-channel convolutions of csrc/elementwise.hip
(encdiff_small_conv_fwd / encdiff_small_conv_bwd), written from the entry points' layouts:

  input conv   x fp32 NCHW [B][ci][h][w]   -> y bf16 rows [B*h*w][ld >= co]
  output conv  x bf16 rows [B*h*w][ld >= ci] -> y fp32 NCHW [B][co][h][w]
  weight [co][ci][3][3], bias [co]; 3x3, stride 1, zero padding 1.

Each function is a loop over the nine taps on a zero-padded copy -- no call into torch's own
convolution, which tests/test_smallconv_restate.py holds it against.  Everything is dtype- and
device-generic: evaluated in fp64 it is the reference, in fp32 the "torch fp32 evaluation" whose
distance from fp64 sets the floor of the per-element rules (tests/elementwise_restate.py).
tests/test_gpu_small_conv.py compares the HIP kernels with it.
"""
import torch
import torch.nn.functional as Fn


def rows_to_nchw(rows, B, h, w):
    """[B*h*w][C] rows (any row stride) -> [B][C][h][w]."""
    return rows.reshape(B, h, w, rows.shape[1]).permute(0, 3, 1, 2)


def nchw_to_rows(x):
    """[B][C][h][w] -> [B*h*w][C]."""
    B, C, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * h * w, C)


def _taps():
    return [(ty, tx) for ty in range(3) for tx in range(3)]


def conv3x3(x, w, b):
    """y[n][co][y][x] = b[co] + sum_{ci, ty, tx} w[co][ci][ty][tx] * x[n][ci][y + ty - 1][x + tx - 1]."""
    B, _, h, wd = x.shape
    xp = Fn.pad(x, (1, 1, 1, 1))
    y = torch.zeros(B, w.shape[0], h, wd, dtype=x.dtype, device=x.device)
    for ty, tx in _taps():
        y = y + torch.einsum("bchw,oc->bohw", xp[:, :, ty:ty + h, tx:tx + wd], w[:, :, ty, tx])
    return y + b.view(1, -1, 1, 1)


def conv3x3_dx(dy, w):
    """dx[n][ci][y][x] = sum_{co, ty, tx} w[co][ci][ty][tx] * dy[n][co][y - ty + 1][x - tx + 1]."""
    B, _, h, wd = dy.shape
    dp = Fn.pad(dy, (1, 1, 1, 1))
    dx = torch.zeros(B, w.shape[1], h, wd, dtype=dy.dtype, device=dy.device)
    for ty, tx in _taps():
        dx = dx + torch.einsum("bohw,oc->bchw", dp[:, :, 2 - ty:2 - ty + h, 2 - tx:2 - tx + wd], w[:, :, ty, tx])
    return dx


def conv3x3_dw(x, dy):
    """dW[co][ci][ty][tx] = sum_{n, y, x} dy[n][co][y][x] * x[n][ci][y + ty - 1][x + tx - 1]."""
    B, ci, h, wd = x.shape
    xp = Fn.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(dy.shape[1], ci, 3, 3, dtype=x.dtype, device=x.device)
    for ty, tx in _taps():
        # added to +0, as the kernels' sums start: never -0
        dw[:, :, ty, tx] += torch.einsum("bohw,bchw->oc", dy, xp[:, :, ty:ty + h, tx:tx + wd])
    return dw


def conv3x3_db(dy):
    """db[co] = sum_{n, y, x} dy[n][co][y][x]."""
    return dy.sum(dim=(0, 2, 3))
