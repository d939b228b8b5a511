"""Record tests/golden/beta_vae_small.npz by running the REFERENCE's beta-VAE score and sklearn on the CPU.

    python tools/gen_golden_beta_vae.py [--out DIR]   record the fixture
    python tools/gen_golden_beta_vae.py --time        time the reference's compute_beta_vae_sklearn and
                                                      eval_func's PCA loop at eval_func's sizes
                                                      (10 000 / 5 000 points of 64 pairs, D = 20;
                                                      tokens 480000 x 20 x 16)

Needs the reference tree and scikit-learn, so it runs only where those exist.  The functions that
run are the reference's own compute_beta_vae_sklearn, _generate_training_batch and
_generate_training_sample (evaluation/metrics/beta_vae.py), behind the gin / absl stand-ins of
gen_golden_metrics.py, sklearn's LogisticRegression and sklearn's PCA.  Data only is stored.

main    grid [4, 3, 5] (N = 60), D = 6 codes, compute_beta_vae_sklearn(batch_size 16, 600 training
        and 400 evaluation points, RandomState(0)).  The index tables are read off the reference's
        run through a recording lookup, the fitted model through a constructor that stands where
        beta_vae.py names linear_model.LogisticRegression and keeps what it builds.
fit_*   direct LogisticRegression().fit cases on tables built here (float32 values, as the feature
        table holds): conv (600, 8, 3), cap (n_iter_ == 100: the first table found that hits it),
        d1 (601, 1, 3), rows (1025, 20, 6), wide (257, 64, 16), zero (600, 8, 4 with an all-zero
        column).
pca_*   sklearn's PCA(n_components=1).fit_transform per unit, as eval_func loops, on the float32
        tokens of tests/logreg_restate.py make_tokens; its error against the float64 restatement is
        recorded, the small tables' outputs in full.

Per case delta = the larger of |centred decision difference| against sklearn of the restatement
(tests/logreg_restate.py) and of the restatement run on row-permuted input: how far the summation
order alone moves the result.  It is measured here and stored, not chosen.  Conditions asserted
before the fixture is written, a table's seed being advanced until they hold:
  * the restatement and its permuted run both give sklearn's n_iter_ (a table on which the permuted
    run stops elsewhere sits on the edge of a stopping test) and end with the matching status;
  * at most 1 % of the rows have a top-two decision margin (sklearn's) of 2 * 8 * delta or less;
  * no restatement prediction differs from sklearn's on the other rows.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import gen_golden_metrics as GM  # noqa: E402
import logreg_restate as R  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
SIZES = [4, 3, 5]
SEED = 0
BATCH, N_TRAIN, N_EVAL = 16, 600, 400
TOL_FACTOR = 8.0
MAX_LEFT_OUT = 0.01
#        name    n     D   K  scale  wanted n_iter_ == 100
CASES = (('conv', 600, 8, 3, 1.0, False), ('cap', 600, 8, 4, 100.0, True), ('d1', 601, 1, 3, 1.0, False),
         ('rows', 1025, 20, 6, 1.0, False), ('wide', 257, 64, 16, 0.25, False), ('zero', 600, 8, 4, 1.0, False))


def main_codes(noise_seed):
    f = GM.all_factors(SIZES).astype(np.float64)
    z = np.random.RandomState(noise_seed).randn(f.shape[0], 6)
    t = np.stack([f[:, 0] / 3 + 0.25 * z[:, 0], f[:, 1] / 2 + 0.25 * z[:, 1], f[:, 2] / 4 + 0.2 * z[:, 2],
                  0.7 * f[:, 2] / 4 + 0.3 * z[:, 3], 0.5 * z[:, 4], np.full(f.shape[0], 1.25)], 1)
    return t.astype(np.float32)


def fit_table(name, n, D, K, scale, seed):
    """Features shaped like the score's: non-negative, the column of the labelled factor smaller."""
    rs = np.random.RandomState(seed)
    y = rs.randint(K, size=n)
    X = np.abs(rs.randn(n, D)) * scale
    for k in range(min(K, D)):
        X[y == k, k] *= 0.3
    if name == 'zero':
        X[:, D - 1] = 0.0
    return X.astype(np.float32), y.astype(np.int32)


def margins(z):
    s = np.sort(z, axis=1)
    return s[:, -1] - s[:, -2]


def measure(X32, y, model, extra=()):
    """delta, n_iter and left-out share of one fitted sklearn model against the restatement; extra:
    further tables (X32, y) the model's decisions are recorded and compared on."""
    X = X32.astype(np.float64)
    K = len(model.classes_)
    r = R.fit(X, y, K)
    perm = np.random.RandomState(12345).permutation(len(y))
    rp = R.fit(X[perm], y[perm], K)
    n_iter = int(model.n_iter_[0])
    want = R.MAX_ITER if n_iter == 100 and r['status'] == R.MAX_ITER else None
    out = dict(ok=r['n_iter'] == n_iter and rp['n_iter'] == n_iter and r['status'] == rp['status'] and
               r['status'] != R.LINE_SEARCH and (want is None or r['status'] == want), n_iter=n_iter, restate=r)
    delta, tables = 0.0, []
    for Xt32, yt in ((X32, y),) + tuple(extra):
        Xt = Xt32.astype(np.float64)
        zs = model.decision_function(Xt)
        for fit_ in (r, rp):
            delta = max(delta, float(np.abs(R.centred(R.decisions(Xt, fit_['coef'], fit_['intercept'])) -
                                            R.centred(zs)).max()))
        tables.append((Xt, yt, zs))
    out['delta'] = delta
    tol = TOL_FACTOR * delta
    for Xt, yt, zs in tables:
        keep = margins(zs) > 2 * tol
        left = 1.0 - keep.mean()
        pred = model.predict(Xt)
        assert np.array_equal(pred, np.argmax(zs, axis=1))
        for fit_ in (r, rp):
            mine = np.argmax(R.decisions(Xt, fit_['coef'], fit_['intercept']), axis=1)
            out['ok'] = out['ok'] and left <= MAX_LEFT_OUT and np.array_equal(mine[keep], pred[keep])
        out.setdefault('left_out', []).append(int((~keep).sum()))
    return out


class Models:
    """Stands where beta_vae.py names linear_model.LogisticRegression: keeps the models it builds."""

    def __init__(self):
        from sklearn.linear_model import LogisticRegression
        self.real, self.made = LogisticRegression, []  # beta_vae.py's linear_model is sklearn's own module

    def __call__(self, **kw):
        self.made.append(self.real(**kw))
        return self.made[-1]


def record_main(res):
    from evaluation.metrics import beta_vae as BV
    ds = GM.ref_grid(SIZES)
    noise_seed = 0
    while True:
        codes = main_codes(noise_seed)
        rep, picks, models = GM.Lookup(codes), [], Models()
        inner, real = BV._generate_training_sample, BV.linear_model.LogisticRegression
        points = []

        def recording(*a, **k):
            out = inner(*a, **k)
            picks.append(out[0])
            points.append(out[1])
            return out

        BV._generate_training_sample, BV.linear_model.LogisticRegression = recording, models
        try:
            scores = BV.compute_beta_vae_sklearn(ds, rep, np.random.RandomState(SEED), None, batch_size=BATCH,
                                                 num_train=N_TRAIN, num_eval=N_EVAL)
        finally:
            BV._generate_training_sample, BV.linear_model.LogisticRegression = inner, real
        seen = np.stack(rep.seen)
        assert seen.shape == (2 * (N_TRAIN + N_EVAL), BATCH) and len(models.made) == 1
        idx1, idx2, labels = seen[0::2].astype(np.int32), seen[1::2].astype(np.int32), np.array(picks, np.int32)
        pts = np.stack(points)
        assert pts.dtype == np.float32  # the reference stores these rows into its float64 table
        pts = pts.astype(np.float64)
        model = models.made[0]
        assert len(model.classes_) == len(SIZES)
        x_tr, x_ev = pts[:N_TRAIN].astype(np.float32), pts[N_TRAIN:].astype(np.float32)
        assert np.array_equal(x_tr.astype(np.float64), pts[:N_TRAIN])  # the features are float32 values
        m = measure(x_tr, labels[:N_TRAIN], model, extra=((x_ev, labels[N_TRAIN:]),))
        if m['ok']:
            break
        print(f'main: noise seed {noise_seed}: delta {m["delta"]:.3g}, left out {m["left_out"]} -- next seed')
        noise_seed += 1
        assert noise_seed < 200, 'main'
    res.update(sizes=np.array(SIZES), seed=np.array(SEED), batch=np.array(BATCH), num_train=np.array(N_TRAIN),
               num_eval=np.array(N_EVAL), noise_seed=np.array(noise_seed), codes=codes,
               train_idx1=idx1[:N_TRAIN], train_idx2=idx2[:N_TRAIN], train_labels=labels[:N_TRAIN],
               eval_idx1=idx1[N_TRAIN:], eval_idx2=idx2[N_TRAIN:], eval_labels=labels[N_TRAIN:],
               train_points=pts[:N_TRAIN], eval_points=pts[N_TRAIN:],
               scores=np.array([scores['train_accuracy'], scores['eval_accuracy']], np.float64),
               main_coef=model.coef_, main_intercept=model.intercept_, main_n_iter=np.array(m['n_iter']),
               main_delta=np.float64(m['delta']), main_left_out=np.array(m['left_out']),
               main_train_decisions=model.decision_function(pts[:N_TRAIN]),
               main_eval_decisions=model.decision_function(pts[N_TRAIN:]))
    print(f'main: noise seed {noise_seed}, scores {scores}, n_iter {m["n_iter"]}, delta {m["delta"]:.3g}, '
          f'left out {m["left_out"]} of ({N_TRAIN}, {N_EVAL}), line search evaluations <= {m["restate"]["max_ls_evals"]}')


def record_fits(res):
    from sklearn.linear_model import LogisticRegression
    names, multi = [], False
    for name, n, D, K, scale, cap in CASES:
        seed = 0
        while True:
            X32, y = fit_table(name, n, D, K, scale, seed)
            model = LogisticRegression().fit(X32.astype(np.float64), y)
            m = measure(X32, y, model)
            if m['ok'] and (m['n_iter'] == 100) == cap and len(model.classes_) == K:
                break
            print(f'fit_{name}: seed {seed}: n_iter {m["n_iter"]} (restated {m["restate"]["n_iter"]}), delta '
                  f'{m["delta"]:.3g}, left out {m["left_out"]} -- next seed')
            seed += 1
            assert seed < 200, name
        p = f'fit_{name}_'
        res.update({p + 'x': X32, p + 'y': y, p + 'coef': model.coef_, p + 'intercept': model.intercept_,
                    p + 'n_iter': np.array(m['n_iter']), p + 'delta': np.float64(m['delta']),
                    p + 'left_out': np.array(m['left_out'][0]), p + 'seed': np.array(seed),
                    p + 'decisions': model.decision_function(X32.astype(np.float64)),
                    p + 'max_ls_evals': np.array(m['restate']['max_ls_evals'])})
        multi = multi or m['restate']['max_ls_evals'] > 1
        names.append(name)
        print(f'fit_{name}: seed {seed}, n_iter {m["n_iter"]}, status {m["restate"]["status"]}, delta {m["delta"]:.3g}, '
              f'left out {m["left_out"][0]} of {n}, line search evaluations <= {m["restate"]["max_ls_evals"]}')
    assert multi, 'no case takes more than one evaluation inside a line search'
    res['fit_cases'] = np.array(names)


def sklearn_pca(tokens):
    from sklearn.decomposition import PCA
    cols, comps = [], []
    for i in range(tokens.shape[1]):
        pca = PCA(n_components=1)
        cols.append(pca.fit_transform(tokens[:, i, :]))
        comps.append(pca.components_[0])
    return np.concatenate(cols, axis=1), np.stack(comps)


def record_pca(res):
    for i, shape in enumerate(R.TOKEN_SHAPES):
        tokens = R.make_tokens(shape)
        ref, comps = sklearn_pca(tokens)
        assert ref.dtype == np.float32
        mine, my_comps, mean, ev = R.token_pca(tokens)
        assert np.all(np.sum(comps * my_comps, axis=1) > 0.999), 'the sign rule differs from sklearn'
        p = f'pca{i}_'
        res.update({p + 'shape': np.array(shape), p + 'sum': np.float64(tokens.astype(np.float64).sum()),
                    p + 'ref_err': np.float64(np.abs(ref.astype(np.float64) - mine).max()),
                    p + 'max_abs': np.float64(np.abs(mine).max()), p + 'components': comps})
        if tokens.size <= 20000:
            res[p + 'codes'] = ref
        print(f'pca {shape}: sklearn float32 error {res[p + "ref_err"]:.3g} at scale {res[p + "max_abs"]:.3g}')


def generate(out_dir):
    import sklearn
    GM.install_stand_ins()
    warnings.simplefilter('ignore')  # ConvergenceWarning of the cap case
    res = dict(sklearn_version=np.array(sklearn.__version__), tol_factor=np.float64(TOL_FACTOR))
    record_main(res)
    record_fits(res)
    record_pca(res)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'beta_vae_small.npz')
    np.savez_compressed(path, **res)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


def time_reference():
    """compute_beta_vae_sklearn and eval_func's PCA loop at eval_func's sizes on synthetic tables."""
    gin = GM.install_stand_ins()
    import data.ground_truth.shapes3d as dshapes3d
    from evaluation.metrics import beta_vae as BV
    sizes = [10, 10, 10, 8, 4, 15]
    f = GM.all_factors(sizes).astype(np.float32)
    rs = np.random.RandomState(0)
    codes = np.concatenate([f / np.array(sizes, np.float32), rs.randn(f.shape[0], 14).astype(np.float32)], 1)
    codes[:, :6] += 0.1 * rs.randn(f.shape[0], 6).astype(np.float32)
    ds = dshapes3d.Dataset(np.arange(480000))
    for k, v in (('num_train', 10000), ('num_eval', 5000), ('batch_size', 64)):
        gin.bind_parameter('beta_vae_sklearn.' + k, v)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = BV.compute_beta_vae_sklearn(ds, lambda x: codes[x], random_state=np.random.RandomState(0), artifact_dir=None)
        times.append(time.perf_counter() - t0)
    print(f'compute_beta_vae_sklearn: {min(times):.3f} s best, {max(times):.3f} s worst of 3 on {os.cpu_count()} CPUs '
          f'-> {out}')
    tokens = R.make_tokens((480000, 20, 16))
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        sklearn_pca(tokens)
        times.append(time.perf_counter() - t0)
    print(f'PCA(n_components=1) over 20 units of (480000, 16): {min(times):.3f} s best, {max(times):.3f} s worst of 3')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--time', action='store_true')
    a = ap.parse_args()
    time_reference() if a.time else generate(a.out)
