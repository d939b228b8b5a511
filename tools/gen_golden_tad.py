"""Record tests/golden/tad_small.npz by running the REFERENCE's aurocs_search on the CPU.

    python tools/gen_golden_tad.py [--out DIR]      record the fixture
    python tools/gen_golden_tad.py --check          record again and compare every array with the
                                                    committed fixture, bit for bit

Needs the reference tree (tools/gen_golden_metrics.py's REF), so it runs only where that exists.  What runs
is the reference's own ae_utils_exp: aurocs_search, aurocs, calculate_auroc and LatentClass, on a
stub model whose cond_stage_model returns a fixed table (context_dim x latent_unit columns, device
"cpu").  The module hard-codes .cuda() and imports tqdm: torch.Tensor.cuda becomes the identity for
the run and a pass-through tqdm of two lines stands in (sys.modules).  Data only is stored: the inputs, the
thresholds torch.arange gives, the reference's aurocs and base rates, and the margins below.

aurocs_search builds its predictions as (N, 40) and compares them with targ, so it takes exactly 40
label columns and loops over 40 attributes; a case with more labels (a64) hands it the first 40,
whose areas do not depend on the others.

Cases, each from a seeded torch generator (draws in the order labels, flips, z):
  main  N = 1031 (prime), L = 6, A = 40.  Labels Bernoulli with rates linspace(0.08, 0.9, 40);
        attribute 5 is attribute 4 with 5 % of the rows flipped.  z standard normal, then column 0
        += 3 attr 3, column 1 -= 2.5 attr 7, column 2 *= 0.02 (range below 0.2: gated), column 3
        rounded to halves (ties on thresholds), column 4 += 3 attr 4, column 5 += attr 3.
  wide  N = 300, L = 65, A = 40: crosses the edge of a 32- and of a 64-column tile.
  a64   N = 130, L = 3, A = 64.

Conditions, asserted here and stored: on every case every |max_auroc - 0.75|, |ent_red_prop - 0.2|
and |column range - 0.2| is >= 1e-3 and every base rate lies strictly inside (0, 1); on main there
is a gated column, a tie z == thr above the lowest threshold (which is the column minimum, a tie in
every column), an attribute removed by each of the two
filters and at least 2 captured.  The script arithmetic (celeba_tad.py:47-120 cannot be imported:
it loads a checkpoint at import) is tests/tad_restate.py's.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from gen_golden_metrics import REF  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
MARGIN = 1e-3

TQDM_STAND_IN = '''
def tqdm(it, *args, **kwargs):
    return it
'''


def import_reference():
    shim = types.ModuleType('tqdm')
    exec(TQDM_STAND_IN, shim.__dict__)
    sys.modules['tqdm'] = shim
    sys.path.insert(0, REF)
    import ae_utils_exp
    return ae_utils_exp


class Table:
    """cond_stage_model of the stub: returns the fixed table whatever it is given."""

    def __init__(self, z):
        self.z, self.context_dim, self.latent_unit = z, z.shape[1], 1

    def __call__(self, data):
        return self.z


class Stub:
    device = 'cpu'

    def __init__(self, z):
        self.cond_stage_model = Table(z)


def run_reference(ae_utils_exp, z, targ):
    """aurocs_search on (z, targ[:, :40]) with .cuda() the identity; (aurocs (40, L), base rates, s)."""
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    t0 = time.perf_counter()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            au, base, _ = ae_utils_exp.aurocs_search(z, targ[:, :40], Stub(z))
    finally:
        torch.Tensor.cuda = saved
    return au.numpy(), base.numpy(), time.perf_counter() - t0


def labels(g, n, a):
    rates = torch.linspace(0.08, 0.9, a)
    return torch.bernoulli(rates.expand(n, a).contiguous(), generator=g).to(torch.int64)


def case_main():
    g = torch.Generator().manual_seed(0)
    n = 1031
    targ = labels(g, n, 40)
    flip = (torch.rand(n, generator=g) < 0.05).to(torch.int64)
    targ[:, 5] = targ[:, 4] ^ flip
    z = torch.randn(n, 6, generator=g)
    z[:, 0] += 3 * targ[:, 3]
    z[:, 1] -= 2.5 * targ[:, 7]
    z[:, 2] *= 0.02
    z[:, 3] = torch.round(z[:, 3] * 2) / 2
    z[:, 4] += 3 * targ[:, 4]
    z[:, 5] += 1 * targ[:, 3]
    return z, targ


def case_wide():
    g = torch.Generator().manual_seed(1)
    n = 300
    targ = labels(g, n, 40)
    z = torch.randn(n, 65, generator=g)
    z[:, 31] += 3 * targ[:, 9]
    z[:, 32] -= 3 * targ[:, 20]
    z[:, 63] += 2.5 * targ[:, 30]
    z[:, 64] -= 3 * targ[:, 12]
    z[:, 40] *= 0.03
    return z, targ


def case_a64():
    g = torch.Generator().manual_seed(2)
    n = 130
    targ = labels(g, n, 64)
    z = torch.randn(n, 3, generator=g)
    z[:, 0] += 3 * targ[:, 50]
    z[:, 1] -= 3 * targ[:, 63]
    z[:, 2] += 3 * targ[:, 10]
    return z, targ


def record(ae_utils_exp, name, z, targ):
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import tad_restate as R
    au, base, secs = run_reference(ae_utils_exp, z, targ)
    zn, tn = z.numpy(), targ.numpy().astype(np.uint8)
    t = torch.arange(0.0, 1.0001, step=0.1).numpy()
    assert au.dtype == np.float32 and au.shape == (40, zn.shape[1]) and t.shape == (11,) and t.dtype == np.float32
    # margins, on the restatement's areas for all attributes (the first 40 are compared with the
    # reference's in tests/test_tad_host.py)
    full = R.aurocs(zn, tn, t)
    assert np.abs(full[:40] - au).max() <= 1e-6, name
    res = R.tad(full, tn)
    ma, mi = R.column_range(zn)
    rng = (ma - mi).astype(np.float64)
    rates = R.base_rates(tn)
    assert np.array_equal(rates[:40], base), name
    thr = R.thresholds(t, ma, mi)
    ungated = rng > 0.2
    ties = int(sum((zn[:, l:l + 1] == thr[l:l + 1, 1:]).sum() for l in np.nonzero(ungated)[0]))
    m = {'margin_auroc': np.abs(res['max_auroc'] - 0.75).min(), 'margin_ent': np.abs(res['ent_red_prop'] - 0.2).min(),
         'margin_range': np.abs(rng - 0.2).min(), 'min_ungated_range': rng[ungated].min(),
         'gated': int((~ungated).sum()), 'ties': ties,
         'by_auroc': int((res['max_auroc'] >= 0.75).sum()),
         'removed_by_ent': int(((res['max_auroc'] >= 0.75) & ~res['captured']).sum()),
         'captured': res['attributes_captured']}
    assert m['margin_auroc'] >= MARGIN and m['margin_ent'] >= MARGIN and m['margin_range'] >= MARGIN, (name, m)
    assert ((rates > 0) & (rates < 1)).all(), name
    if name == 'main':
        assert m['gated'] >= 1 and m['ties'] >= 1 and m['removed_by_ent'] >= 1 and m['captured'] >= 2, m
        assert m['by_auroc'] < 40  # the other filter removes some too
    out = {f'{name}_z': zn, f'{name}_targ': tn, f'{name}_aurocs': au, f'{name}_base_rates': base}
    out.update({f'{name}_{k}': np.asarray(v) for k, v in m.items()})
    print(f'{name}: N={zn.shape[0]} L={zn.shape[1]} A={tn.shape[1]}: reference {secs:.1f} s; restatement within '
          f'{np.abs(full[:40] - au).max():.2e}; TAD {res["tad_score"]:.4f}, captured '
          f'{np.nonzero(res["captured"])[0].tolist()}, max_auroc >= 0.75 at '
          f'{np.nonzero(res["max_auroc"] >= 0.75)[0].tolist()}; ' + ', '.join(f'{k} {v:.4g}' for k, v in m.items()))
    return out


def generate():
    ref = import_reference()
    res = {'t': torch.arange(0.0, 1.0001, step=0.1).numpy()}
    for name, make in (('main', case_main), ('wide', case_wide), ('a64', case_a64)):
        res.update(record(ref, name, *make()))
    return res


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--check', action='store_true')
    a = ap.parse_args()
    res = generate()
    path = os.path.join(a.out, 'tad_small.npz')
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
