"""Float64 numpy restatement of the reference's reconstruction scores, written from the formulas of
recon_metrics.py (_ssim, calculate_ssim, calculate_mse), not from csrc/recon.hip or
encdiff_amd/metrics.py.  Inputs and the 121 window weights are taken as the float32 values the
reference has; everything after them is float64: the five moments are zero-padded 121-tap sums, so
sigma = conv(a a) - mu^2 does not cancel in float32 as the reference's does.
tests/test_recon_host.py checks it against the reference's own output (tests/golden/recon_small.npz,
tools/gen_golden_recon.py) within the deviation recorded per case; the GPU tests compare the kernel
with it.
"""
import numpy as np

F32, F64 = np.float32, np.float64
WINDOW = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2


def from_u8(u):
    """uint8 pixels -> float32 in [-1, 1] as the data pipeline does (x / 127.5 - 1), the quotient and
    the difference rounded to float32 one by one.  The fixture stores its images as uint8."""
    return ((np.asarray(u).astype(F32) / F32(127.5)).astype(F32) - F32(1.0)).astype(F32)


def premap(x, pre_add=1.0, pre_mul=0.5):
    """(x + pre_add) * pre_mul in float32, sum and product rounded one by one: the script's
    (x + 1.) / 2. at the defaults (halving is exact in binary)."""
    x = np.asarray(x, F32)
    return ((x + F32(pre_add)).astype(F32) * F32(pre_mul)).astype(F32)


def window_sum(x, window):
    """F.conv2d(x, window, padding=5, groups=Ch) of _ssim in float64: (B, Ch, H, W) -> the same shape,
    out[y][x] = sum_{dy, dx} window[dy][dx] * in[y + dy - 5][x + dx - 5], zero outside the plane."""
    x, window = np.asarray(x, F64), np.asarray(window, F64)
    r = WINDOW // 2
    h, w = x.shape[2:]
    pad = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)))
    taps = [window[dy, dx] * pad[:, :, dy:dy + h, dx:dx + w] for dy in range(WINDOW) for dx in range(WINDOW)]
    return np.sum(np.stack(taps), axis=0)


def ssim_map(a, b, window):
    """_ssim:10-24 before the mean, float64, (B, Ch, H, W)."""
    a, b = np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64)
    mu1, mu2 = window_sum(a, window), window_sum(b, window)
    s1 = window_sum(a * a, window) - mu1 * mu1
    s2 = window_sum(b * b, window) - mu2 * mu2
    s12 = window_sum(a * b, window) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim(a, b, window):
    """calculate_ssim: float64 (B,), the mean over Ch, H, W."""
    return ssim_map(a, b, window).mean(axis=(1, 2, 3))


def mse(a, b):
    """calculate_mse: float64 (B,), (a - b)^2 averaged over Ch, H, W."""
    d = np.asarray(a, F32).astype(F64) - np.asarray(b, F32).astype(F64)
    return (d * d).mean(axis=(1, 2, 3))
