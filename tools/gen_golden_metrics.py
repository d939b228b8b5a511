"""Record tests/golden/metrics_small.npz by running the REFERENCE's metric functions on the CPU.

    python tools/gen_golden_metrics.py [--out DIR]      record the fixture
    python tools/gen_golden_metrics.py --time           time the reference's compute_factor_vae and
                                                        compute_mig at eval_func's sizes on a
                                                        synthetic (480000, 20) Shapes3D table

Needs the reference tree (tools/gen_golden.py's REF), so it runs only where that exists.  The
functions that run are the reference's own: compute_factor_vae, _generate_training_batch,
_compute_variances (evaluation/metrics/factor_vae.py), compute_mig (mig.py), _histogram_discretize,
discrete_mutual_info, discrete_entropy, generate_batch_factor_code (utils.py) and the ground-truth
classes of data/ground_truth.  Their modules import gin and absl; two stand-in modules of a few lines
are written into a temporary directory (gin: configurable with bind_parameter, REQUIRED;
absl.logging).  Data only is stored: inputs, the index tables the reference drew, and its results.

The index tables are read off the reference's run: its "observations" are dataset indices
(Dataset(np.arange(N))) and its representation function is the row lookup codes[x], so a recording
lookup sees every index batch; the factor choice and argmin of each vote are read by wrapping
_generate_training_sample.

Main case: grid [4, 3, 5, 2] (N = 120), D = 7: dimensions 0, 1, 2, 4 carry factors 0, 1, 2, 3,
dimension 3 shares factor 2 with dimension 2, dimension 5 is pure noise and dimension 6 has a
standard deviation of about 0.01 (pruned at 0.05: the compacted index).  FactorVAE at batch 16 and
64, 300 training and 200 evaluation votes, 200 rows of variance estimate; MIG at 500 rows.
Wide case: grid [2, 183], D = 3 with one constant column, MIG at M = 15, 16, 17, 500.

Two conditions on the main case are checked here and stored (min_rel_gap, min_thr_dist): for every
vote the relative gap between the smallest and second-smallest float64 ratio is >= 1e-4 (the
reference's float32 variances then pick the mathematically right argmin), and no sqrt(global
variance) lies within 1e-3 of the threshold.  The table's noise seed is advanced until the reference
alone meets both.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = '/root/reference'
OUT = os.path.join(REPO, 'tests', 'golden')

THRESHOLD = 0.05
SIZES = [4, 3, 5, 2]
WIDE_SIZES = [2, 183]
SEED = 0

GIN_STAND_IN = '''
import functools
REQUIRED = object()
_BOUND = {}


def bind_parameter(name, value):
    _BOUND[name] = value


def configurable(name=None, **_):
    def deco(fn, scope=None):
        scope = scope or fn.__name__

        @functools.wraps(fn)
        def wrapped(*args, **kwargs):
            for key, value in _BOUND.items():
                s, p = key.rsplit('.', 1)
                if s == scope:
                    kwargs.setdefault(p, value)
            return fn(*args, **kwargs)
        return wrapped
    if callable(name):
        return deco(name)
    return lambda fn: deco(fn, name)
'''

ABSL_LOGGING_STAND_IN = '''
def info(*args, **kwargs):
    pass
'''


def install_stand_ins():
    d = tempfile.mkdtemp(prefix='metrics_shims_')
    with open(os.path.join(d, 'gin.py'), 'w') as f:
        f.write(GIN_STAND_IN)
    os.makedirs(os.path.join(d, 'absl'))
    open(os.path.join(d, 'absl', '__init__.py'), 'w').close()
    with open(os.path.join(d, 'absl', 'logging.py'), 'w') as f:
        f.write(ABSL_LOGGING_STAND_IN)
    sys.path.insert(0, d)
    sys.path.insert(0, REF)
    import gin
    from evaluation.metrics import utils
    # eval_func's bindings (main_val.py:74-91)
    gin.bind_parameter('prune_dims.threshold', THRESHOLD)
    gin.bind_parameter('discretizer.discretizer_fn', utils._histogram_discretize)
    gin.bind_parameter('discretizer.num_bins', 20)
    return gin


def ref_grid(sizes):
    """The reference's Shapes3D ground truth (every factor latent, index = factors . bases) with
    other factor sizes: its own class and methods, the size attributes replaced."""
    import data.ground_truth.shapes3d as dshapes3d
    from data.ground_truth import util
    n = int(np.prod(sizes))
    ds = dshapes3d.Dataset(np.arange(n))
    ds.factor_sizes = list(sizes)
    ds.latent_factor_indices = list(range(len(sizes)))
    ds.num_total_factors = len(sizes)
    ds.state_space = util.SplitDiscreteStateSpace(ds.factor_sizes, ds.latent_factor_indices)
    ds.factor_bases = np.prod(ds.factor_sizes) / np.cumprod(ds.factor_sizes)
    return ds


def all_factors(sizes):
    return np.stack(np.unravel_index(np.arange(int(np.prod(sizes))), sizes), 1)


def main_table(noise_seed):
    f = all_factors(SIZES).astype(np.float64)
    rs = np.random.RandomState(noise_seed)
    z = rs.randn(f.shape[0], 7)
    t = np.stack([f[:, 0] / 3 + 0.35 * z[:, 0],
                  f[:, 1] / 2 + 0.35 * z[:, 1],
                  f[:, 2] / 4 + 0.30 * z[:, 2],
                  0.7 * f[:, 2] / 4 + 0.30 * z[:, 3],
                  f[:, 3] + 0.45 * z[:, 4],
                  0.5 * z[:, 5],
                  0.01 * z[:, 6]], 1)
    return t.astype(np.float32)


def wide_table():
    f = all_factors(WIDE_SIZES).astype(np.float64)
    rs = np.random.RandomState(7)
    z = rs.randn(f.shape[0], 3)
    t = np.stack([f[:, 1] / 182 + 0.05 * z[:, 0], np.full(f.shape[0], 1.25), f[:, 0] + 0.3 * z[:, 2]], 1)
    return t.astype(np.float32)


class Lookup:
    """The representation function of eval_func, codes[x], recording every x."""

    def __init__(self, codes):
        self.codes, self.seen = codes, []

    def __call__(self, x):
        self.seen.append(np.array(x, dtype=np.int64))
        return self.codes[x]


def record_fvae(ds, codes, batch):
    """One compute_factor_vae run (RandomState(SEED)); the tables and per-vote results it produced."""
    from evaluation.metrics import factor_vae as FV
    rep, picks = Lookup(codes), []
    inner = FV._generate_training_sample

    def recording(*a, **k):
        out = inner(*a, **k)
        picks.append(out)
        return out

    n_var, n_train, n_eval = 200, 300, 200
    FV._generate_training_sample = recording
    try:
        scores = FV.compute_factor_vae(ds, rep, np.random.RandomState(SEED), None, batch_size=batch,
                                       num_train=n_train, num_eval=n_eval, num_variance_estimate=n_var)
    finally:
        FV._generate_training_sample = inner
    n_chunks = -(-n_var // 64)
    var_idx = np.concatenate(rep.seen[:n_chunks])
    votes_idx = np.stack(rep.seen[n_chunks:])
    assert var_idx.shape == (n_var,) and votes_idx.shape == (n_train + n_eval, batch) and len(picks) == n_train + n_eval
    factor = np.array([p[0] for p in picks])
    argmin = np.array([p[1] for p in picks])
    # the reference's own pieces on the recorded tables
    rs = np.random.RandomState(SEED)
    gvar = FV._compute_variances(ds, Lookup(codes), n_var, rs)
    active = FV._prune_dims(gvar)
    tv = FV._generate_training_batch(ds, Lookup(codes), batch, n_train, rs, gvar, active)
    ev = FV._generate_training_batch(ds, Lookup(codes), batch, n_eval, rs, gvar, active)
    for v, sl in ((tv, slice(0, n_train)), (ev, slice(n_train, None))):
        chk = np.zeros_like(v)
        np.add.at(chk, (factor[sl], argmin[sl]), 1)
        assert np.array_equal(chk, v)
    # float64 margins of this run
    g64 = np.var(codes[var_idx].astype(np.float64), axis=0, ddof=1)
    act64 = np.sqrt(g64) >= THRESHOLD
    assert np.array_equal(act64, active)
    thr_dist = np.abs(np.sqrt(g64) - THRESHOLD).min()
    ratio = np.var(codes[votes_idx].astype(np.float64), axis=1, ddof=1)[:, act64] / g64[act64]
    srt = np.sort(ratio, axis=1)
    gap = ((srt[:, 1] - srt[:, 0]) / srt[:, 1]).min()
    agree = np.array_equal(np.argmin(ratio, axis=1), argmin)
    p = f'fvae{batch}_'
    res = {p + 'var_idx': var_idx.astype(np.int32), p + 'global_var': np.asarray(gvar),
           p + 'active': active, p + 'train_idx': votes_idx[:n_train].astype(np.int32),
           p + 'train_factor': factor[:n_train].astype(np.int32), p + 'train_argmin': argmin[:n_train].astype(np.int32),
           p + 'train_votes': tv, p + 'eval_idx': votes_idx[n_train:].astype(np.int32),
           p + 'eval_factor': factor[n_train:].astype(np.int32), p + 'eval_argmin': argmin[n_train:].astype(np.int32),
           p + 'eval_votes': ev,
           p + 'scores': np.array([scores['train_accuracy'], scores['eval_accuracy'], scores['num_active_dims']],
                                  dtype=np.float64)}
    return res, gap, thr_dist, agree


def record_mig(ds, codes, m, prefix):
    from evaluation.metrics import mig as MIG, utils
    rep = Lookup(codes)
    mus, ys = utils.generate_batch_factor_code(ds, rep, m, np.random.RandomState(SEED), 16)
    idx = np.concatenate(rep.seen)
    assert mus.shape == (codes.shape[1], m) and np.array_equal(mus.T, codes[idx])
    bins = utils._histogram_discretize(mus, 20)
    edges = np.stack([np.histogram(mus[i], 20)[1][:-1] for i in range(mus.shape[0])])
    assert edges.dtype == np.float32
    mi = utils.discrete_mutual_info(bins, ys)
    h = utils.discrete_entropy(ys)
    score = MIG.compute_mig(ds, Lookup(codes), np.random.RandomState(SEED), None, num_train=m)['discrete_mig']
    assert score == MIG._compute_mig(mus, ys)['discrete_mig']
    return {prefix + 'idx': idx.astype(np.int32), prefix + 'factors': ys.astype(np.int32),
            prefix + 'edges': edges, prefix + 'bins': bins.astype(np.int32), prefix + 'mi': mi, prefix + 'h': h,
            prefix + 'score': np.float64(score)}


def named_grid_checks():
    """(factors, index) samples of the reference's Shapes3D, MPI3D and Cars3D ground truths."""
    import data.ground_truth.mpi3d as dmpi3d
    import data.ground_truth.shapes3d as dshapes3d
    res = {}
    rs = np.random.RandomState(3)
    for name, mod, n in (('shapes3d', dshapes3d, 480000), ('mpi3d', dmpi3d, 1036800)):
        ds = mod.Dataset(np.arange(n))
        f = ds.sample_factors(64, rs)
        f[0], f[1] = 0, np.array(ds.factor_sizes) - 1
        res[name + '_factors'] = f
        res[name + '_index'] = ds.sample_observations_from_factors(f, rs).astype(np.int64)
        res[name + '_sizes'] = np.array(ds.factor_sizes)
    import data.ground_truth.cars3d as dcars3d
    ds = dcars3d.Dataset(np.arange(17568))
    f = all_factors(ds.factor_sizes)
    # the lookup of cars3d is the identity on the row-major enumeration: the same mixed radix
    assert np.array_equal(ds.sample_observations_from_factors(f, rs), np.arange(17568))
    res['cars3d_sizes'] = np.array(ds.factor_sizes)
    return res


def generate(out_dir):
    install_stand_ins()
    ds = ref_grid(SIZES)
    noise_seed = 0
    while True:
        codes = main_table(noise_seed)
        res = dict(sizes=np.array(SIZES), codes=codes, seed=np.array(SEED), threshold=np.array(THRESHOLD),
                   noise_seed=np.array(noise_seed), numpy_major=np.array(int(np.__version__.split('.')[0])))
        gaps, dists, ok = [], [], True
        for batch in (16, 64):
            r, gap, dist, agree = record_fvae(ds, codes, batch)
            res.update(r)
            gaps.append(gap)
            dists.append(dist)
            ok = ok and agree
        if ok and min(gaps) >= 1e-4 and min(dists) >= 1e-3:
            break
        print(f'noise seed {noise_seed}: gap {min(gaps):.3g}, threshold distance {min(dists):.3g}, '
              f'float32 argmin agrees: {ok} -- next seed')
        noise_seed += 1
    res['min_rel_gap'], res['min_thr_dist'] = np.float64(min(gaps)), np.float64(min(dists))
    res.update(record_mig(ds, codes, 500, 'mig_'))
    wide = wide_table()
    res['wide_sizes'], res['wide_codes'] = np.array(WIDE_SIZES), wide
    dsw = ref_grid(WIDE_SIZES)
    for m in (15, 16, 17, 500):
        res.update(record_mig(dsw, wide, m, f'wide{m}_'))
    res.update(named_grid_checks())
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'metrics_small.npz')
    np.savez_compressed(path, **res)
    print(f'wrote {path} ({os.path.getsize(path)} bytes): noise seed {noise_seed}, min relative ratio gap '
          f'{min(gaps):.3g}, min |sqrt(var) - {THRESHOLD}| {min(dists):.3g}')
    for b in (16, 64):
        print(f'  batch {b}: scores {res[f"fvae{b}_scores"]}, active {res[f"fvae{b}_active"].astype(int)}')
    print(f'  mig {res["mig_score"]:.6f}; wide ' + ', '.join(f'{res[f"wide{m}_score"]:.6f}' for m in (15, 16, 17, 500)))


def time_reference():
    """The reference's two functions at eval_func's sizes on a synthetic Shapes3D-sized table."""
    gin = install_stand_ins()
    import data.ground_truth.shapes3d as dshapes3d
    from evaluation.metrics import factor_vae as FV, mig as MIG
    sizes = [10, 10, 10, 8, 4, 15]
    f = all_factors(sizes).astype(np.float32)
    rs = np.random.RandomState(0)
    codes = np.concatenate([f / np.array(sizes, np.float32), rs.randn(f.shape[0], 14).astype(np.float32)], 1)
    codes[:, :6] += 0.1 * rs.randn(f.shape[0], 6).astype(np.float32)
    ds = dshapes3d.Dataset(np.arange(480000))
    for k, v in (('num_variance_estimate', 10000), ('num_train', 10000), ('num_eval', 5000), ('batch_size', 64)):
        gin.bind_parameter('factor_vae_score.' + k, v)
    gin.bind_parameter('mig.num_train', 10000)
    rep = lambda x: codes[x]  # noqa: E731
    for name, fn in (('compute_factor_vae', FV.compute_factor_vae), ('compute_mig', MIG.compute_mig)):
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn(ds, rep, random_state=np.random.RandomState(0), artifact_dir=None)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(f'{name}: best of 3 {best:.3f} s on {os.cpu_count()} CPUs (numpy {np.__version__}) -> {out}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--time', action='store_true')
    a = ap.parse_args()
    time_reference() if a.time else generate(a.out)
