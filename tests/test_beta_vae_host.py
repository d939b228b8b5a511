"""CPU tests of the host half of the beta-VAE score and of the token PCA, and of their numpy
restatement tests/logreg_restate.py, against what the reference and sklearn produced
(tests/golden/beta_vae_small.npz, recorded by tools/gen_golden_beta_vae.py).

Bounds.  Index tables and features: exact.  The fit: sklearn's n_iter_ exactly; the centred
decisions (each row's decisions minus their mean over the classes, which removes the free common
shift of the intercepts) within the case's delta, which the generator measured as the larger error
of the restatement and of the restatement on row-permuted input.  Parameters: centred over the
classes likewise, column k of the difference solves [X 1] dtheta = dz with |dz| <= delta per row, so
|dtheta|_2 <= sqrt(n) delta / sigma_min([X 1]) over the columns of X that are not all zero; the
coefficients of an all-zero column stay exactly 0 on both sides (their gradient is l2 w).
"""
import os

import numpy as np
import pytest

import logreg_restate as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_vae_small.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


def fit_cases(gold):
    yield "main", gold["train_points"], gold["train_labels"], {k: gold["main_" + k] for k in
                                                                ("coef", "intercept", "n_iter", "delta")} | \
        {"decisions": gold["main_train_decisions"]}
    for name in gold["fit_cases"]:
        p = f"fit_{name}_"
        yield str(name), gold[p + "x"].astype(np.float64), gold[p + "y"], {k: gold[p + k] for k in
                                                                           ("coef", "intercept", "n_iter", "delta",
                                                                            "decisions")}


def test_sampler_matches_reference(gold, M):
    """One RandomState gives the training table, then the evaluation table, as the reference drew them."""
    sizes, B = gold["sizes"], int(gold["batch"])
    for sample in (lambda rs, n: M.sample_beta_vae(M.FactorGrid(sizes), rs, B, n),
                   lambda rs, n: R.sample_beta_vae(sizes, rs, B, n)):
        rs = np.random.RandomState(int(gold["seed"]))
        for part, n in (("train", int(gold["num_train"])), ("eval", int(gold["num_eval"]))):
            idx1, idx2, labels = sample(rs, n)
            assert idx1.dtype == idx2.dtype == labels.dtype == np.int32 and idx1.shape == (n, B)
            assert np.array_equal(idx1, gold[part + "_idx1"]) and np.array_equal(idx2, gold[part + "_idx2"])
            assert np.array_equal(labels, gold[part + "_labels"])


def test_features_bit_equal(gold):
    for part in ("train", "eval"):
        got = R.features(gold["codes"], gold[part + "_idx1"], gold[part + "_idx2"])
        assert got.dtype == np.float64 and np.array_equal(got, gold[part + "_points"])
    assert not gold["train_points"][:, 5].any()  # the constant code column: an all-zero feature


def test_fit_matches_sklearn(gold):
    multi = 0
    for name, X, y, ref in fit_cases(gold):
        K = ref["coef"].shape[0]
        r = R.fit(X, y, K)
        multi = max(multi, r["max_ls_evals"])
        delta = float(ref["delta"])
        assert r["n_iter"] == int(ref["n_iter"]), name
        assert r["status"] != R.LINE_SEARCH and (r["status"] == R.MAX_ITER) <= (r["n_iter"] == 100), name
        # the record is consistent: sklearn's decisions are its parameters applied
        assert np.allclose(R.decisions(X, ref["coef"], ref["intercept"]), ref["decisions"], rtol=0, atol=1e-9)
        z, pred = R.predict(X, r["coef"], r["intercept"])
        err = np.abs(R.centred(z) - R.centred(ref["decisions"])).max()
        print(f"{name}: n_iter {r['n_iter']}, centred decision error {err:.3g} (delta {delta:.3g})")
        assert err <= delta, name
        s = np.sort(ref["decisions"], axis=1)
        keep = s[:, -1] - s[:, -2] > 2 * float(gold["tol_factor"]) * delta
        assert (~keep).mean() <= 0.01 and np.array_equal(pred[keep], np.argmax(ref["decisions"], axis=1)[keep])
        live = np.abs(X).max(axis=0) > 0
        assert not r["coef"][:, ~live].any() and not ref["coef"][:, ~live].any()
        A = np.concatenate([X[:, live], np.ones((len(y), 1))], 1)
        bound = np.sqrt(len(y)) * delta / np.linalg.svd(A, compute_uv=False)[-1]
        mine = np.concatenate([r["coef"][:, live], r["intercept"][:, None]], 1)
        theirs = np.concatenate([ref["coef"][:, live], ref["intercept"][:, None]], 1)
        d = (mine - mine.mean(0)) - (theirs - theirs.mean(0))
        assert np.linalg.norm(d, axis=1).max() <= bound, name
    assert multi > 1, "no case takes more than one evaluation inside a line search"
    assert 100 in [int(ref["n_iter"]) for _, _, _, ref in fit_cases(gold)]


def test_score_restated(gold):
    """The restated pipeline gives the accuracies compute_beta_vae_sklearn returned (no row of the
    main case lies under the margin: main_left_out is 0 for both tables)."""
    assert not gold["main_left_out"].any()
    r = R.fit(gold["train_points"], gold["train_labels"], len(gold["sizes"]))
    acc = [np.mean(R.predict(gold[p + "_points"], r["coef"], r["intercept"])[1] == gold[p + "_labels"])
           for p in ("train", "eval")]
    assert acc == gold["scores"].tolist()


def test_line_search_failure_is_a_status():
    """A budget of one evaluation per search cannot finish the first search of this table (it takes
    two): the fit ends with status 3 instead of going on."""
    rs = np.random.RandomState(0)
    y = rs.randint(3, size=200)
    X = np.abs(rs.randn(200, 4)) * 30
    full = R.fit(X, y, 3)
    assert full["max_ls_evals"] >= 2 and full["status"] != R.LINE_SEARCH
    saved, R.MAXLS = R.MAXLS, 1
    try:
        assert R.fit(X, y, 3)["status"] == R.LINE_SEARCH
    finally:
        R.MAXLS = saved


def test_pca_sign_rule_and_restatement(gold, M):
    for i, shape in enumerate(R.TOKEN_SHAPES):
        p = f"pca{i}_"
        assert tuple(gold[p + "shape"]) == shape
        tokens = R.make_tokens(shape)
        assert tokens.astype(np.float64).sum() == float(gold[p + "sum"]), "make_tokens no longer gives the recorded table"
        codes, comps, mean, ev = R.token_pca(tokens)
        ref_comps = gold[p + "components"]
        # sklearn's sign: the entry of largest magnitude is positive -- and so is the restatement's
        for c in (ref_comps, comps):
            assert (c[np.arange(shape[1]), np.argmax(np.abs(c), axis=1)] > 0).all()
        assert np.abs(comps - ref_comps).max() <= 1e-5  # float32 eigenvectors of a clearly separated top value
        if p + "codes" in gold:
            assert np.abs(codes - gold[p + "codes"]).max() <= float(gold[p + "ref_err"])
        # the package's host step is the restatement's
        m, cov = R.token_moments(tokens)
        got_c, got_ev = M.token_components(cov)
        assert np.array_equal(got_c, comps) and np.array_equal(got_ev, ev)
    assert np.array_equal(M.pca_sign(np.array([0.5, -2.0, 1.0])), np.array([-0.5, 2.0, -1.0]))
    assert np.array_equal(M.pca_sign(np.array([-1.0, 1.0])), np.array([1.0, -1.0]))  # the first of equals decides
