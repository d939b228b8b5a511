"""Record tests/golden/recon_small.npz by running the REFERENCE's calculate_ssim, create_window and
calculate_mse on the CPU.

    python tools/gen_golden_recon.py [--out DIR]    record the fixture
    python tools/gen_golden_recon.py --check        record again and compare every array with the
                                                    committed fixture, bit for bit

Needs the reference tree (tools/gen_golden_metrics.py's REF), so it runs only where that exists.
recon_metrics.py cannot be imported: from its line 50 on it imports lpips and loads a checkpoint.
The recorder reads the file at run time and executes, in memory, only the part above
"from typing import List" -- the functions -- with the pass-through tqdm of gen_golden_tad.py
standing in (sys.modules).  None of that text is written anywhere; data only is stored.

Cases.  The noisy ones are stored as uint8 (n, ch, h, w) pairs: a is smoothed uniform noise, b is a
plus Gaussian noise of 12 grey levels, both from RandomState(seed).  They become float32 in [-1, 1]
by tests/recon_restate.py from_u8 and then the script's (x + 1.) / 2., and the reference scores
that.  The shapes are those of tests/test_gpu_recon.py: the reference layout (64 planes of 64 x 3,
narrower than the window), nchw, no tile multiple, single pixels, one window, several ragged tiles,
exactly one tile, a flat wide plane.  The two constant cases (images 0.7 and 0.63, given as they
are) are stored as their shape and the two values.

Per case: the reference's float32 ssim and mse per image, the float64 restatement's
(tests/recon_restate.py), and d_ssim / d_mse = max |reference - restatement|.  That deviation is
the reference's own float32 rounding; on the noisy cases it is asserted <= 1e-6 here, on the
constant ones -- where conv(a a) - mu^2 cancels in float32 -- it is only recorded.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from gen_golden_metrics import REF  # noqa: E402
from gen_golden_tad import TQDM_STAND_IN  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
CUT = 'from typing import List'
NOISY = [  # name, (n, ch, h, w), seed
    ('ref_layout', (2, 64, 64, 3), 0), ('nchw', (2, 3, 64, 64), 1), ('ragged', (3, 2, 17, 23), 2),
    ('pixel', (2, 5, 1, 1), 3), ('window', (1, 1, 11, 11), 4), ('tiles', (2, 1, 40, 70), 5),
    ('one_tile', (1, 3, 16, 16), 6), ('flat_wide', (5, 1, 5, 33), 7),
]
CONST = [('const_nchw', (4, 3, 64, 64)), ('const_ref', (4, 64, 64, 3))]
CONST_VALUES = (0.7, 0.63)
BOUND = 1e-6


def import_reference():
    """The functions of recon_metrics.py (everything above CUT), executed in a module of their own."""
    shim = types.ModuleType('tqdm')
    exec(TQDM_STAND_IN, shim.__dict__)
    sys.modules['tqdm'] = shim
    with open(os.path.join(REF, 'recon_metrics.py')) as f:
        text = f.read()
    assert CUT in text, 'recon_metrics.py changed: the line the functions end at is gone'
    mod = types.ModuleType('recon_metrics_functions')
    exec(compile(text[:text.index(CUT)], 'recon_metrics.py', 'exec'), mod.__dict__)
    return mod


def noisy_pair(shape, seed):
    rs = np.random.RandomState(seed)
    x = rs.rand(*shape)
    smooth = sum(np.roll(x, (dy, dx), axis=(2, 3)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    smooth = (smooth - smooth.min()) / max(smooth.max() - smooth.min(), 1e-9)
    a = np.rint(smooth * 255).astype(np.uint8)
    b = np.clip(np.rint(a + rs.normal(0.0, 12.0, shape)), 0, 255).astype(np.uint8)
    return a, b


def score(ref, R, window, a, b):
    """a, b: float32 images in [0, 1] as the reference's functions get them."""
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    ssim_ref, mse_ref = ref.calculate_ssim(ta, tb).numpy(), ref.calculate_mse(ta, tb).numpy()
    assert ssim_ref.dtype == np.float32 and mse_ref.dtype == np.float32 and ssim_ref.shape == (a.shape[0],)
    ssim64, mse64 = R.ssim(a, b, window), R.mse(a, b)
    return {'ssim_ref': ssim_ref, 'mse_ref': mse_ref, 'ssim_f64': ssim64, 'mse_f64': mse64,
            'd_ssim': np.abs(ssim_ref.astype(np.float64) - ssim64).max(),
            'd_mse': np.abs(mse_ref.astype(np.float64) - mse64).max()}


def generate():
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import recon_restate as R
    torch.set_num_threads(1)
    ref = import_reference()
    window = ref.create_window(11, 1)[0, 0].numpy()
    assert window.dtype == np.float32 and window.shape == (11, 11)
    res = {'window': window, 'cases': np.array([c[0] for c in NOISY]), 'const_cases': np.array([c[0] for c in CONST]),
           'const_values': np.array(CONST_VALUES, np.float32)}
    for name, shape, seed in NOISY:
        a, b = noisy_pair(shape, seed)
        out = score(ref, R, window, R.premap(R.from_u8(a)), R.premap(R.from_u8(b)))
        assert out['d_ssim'] <= BOUND and out['d_mse'] <= BOUND, (name, out['d_ssim'], out['d_mse'])
        res.update({f'{name}_a': a, f'{name}_b': b})
        res.update({f'{name}_{k}': np.asarray(v) for k, v in out.items()})
        print(f'{name}: {shape}: ssim {out["ssim_ref"].mean():.4f}, mse {out["mse_ref"].mean():.5f}; reference vs '
              f'float64 restatement: ssim {out["d_ssim"]:.2e}, mse {out["d_mse"]:.2e}')
    for name, shape in CONST:
        a = np.full(shape, CONST_VALUES[0], np.float32)
        b = np.full(shape, CONST_VALUES[1], np.float32)
        out = score(ref, R, window, a, b)
        res[f'{name}_shape'] = np.array(shape, np.int64)
        res.update({f'{name}_{k}': np.asarray(v) for k, v in out.items()})
        print(f'{name}: {shape}: ssim {out["ssim_ref"].mean():.6f} (float64 {out["ssim_f64"].mean():.6f}); '
              f'reference vs float64 restatement: ssim {out["d_ssim"]:.2e}, mse {out["d_mse"]:.2e} (recorded, not bounded)')
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--check', action='store_true')
    a = ap.parse_args()
    res = generate()
    path = os.path.join(a.out, 'recon_small.npz')
    if a.check:
        old = dict(np.load(path))
        assert sorted(old) == sorted(res), 'keys differ'
        for k in res:
            assert old[k].dtype == res[k].dtype and old[k].tobytes() == res[k].tobytes(), k
        print(f'{path}: {len(res)} arrays regenerate bit for bit')
    else:
        os.makedirs(a.out, exist_ok=True)
        np.savez_compressed(path, **res)
        print(f'wrote {path} ({os.path.getsize(path)} bytes)')
