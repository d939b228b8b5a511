"""GPU tests of the beta-VAE kernels (csrc/beta_vae.hip) and of metrics.beta_vae_score, against the
numpy restatement tests/logreg_restate.py on the same inputs and against what sklearn and the
reference's compute_beta_vae_sklearn produced (tests/golden/beta_vae_small.npz, recorded by
tools/gen_golden_beta_vae.py).

Bounds.  Features: exactly equal -- float32 sums in the reference's order.  The fit: sklearn's n_iter_
exactly, and sklearn's prediction on every row whose recorded top-two decision margin exceeds 2 *
tol_case, tol_case = 8 * delta_case; delta_case is what the generator measured for the restatement
and for its row-permuted run, the factor 8 is there because the device's reduction tree differs from
both host orders.  The generator asserted that at most 1 % of a case's rows fall under the margin.
The centred decision difference against sklearn is printed beside tol_case for every case.  Two
launches give identical bits.  The score: within (rows left out) / n of the reference's.
"""
import os

import numpy as np
import pytest
import torch

import logreg_restate as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_vae_small.npz")
F64, F32, I32 = torch.float64, torch.float32, torch.int32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


@pytest.fixture(scope="module")
def ops():
    from encdiff_amd import ops
    return ops


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ features
@pytest.mark.parametrize("D", [1, 8, 20, 64])
def test_features_exact(ops, D):
    sizes = [4, 3, 5]
    codes = (np.random.RandomState(D).randn(60, D) * np.linspace(0.01, 30, D)).astype(np.float32)
    for B in (2, 37, 64):
        for P in (1, 257):
            idx1, idx2, _ = R.sample_beta_vae(sizes, np.random.RandomState(B * 1000 + P), B, P)
            out = torch.full((P, D), -1.0, device="cuda", dtype=F64)
            ops.beta_features(up(codes), up(idx1), up(idx2), out)
            assert np.array_equal(out.cpu().numpy(), R.features(codes, idx1, idx2)), (D, B, P)


# ------------------------------------------------------------------ the fit
def device_fit(ops, X, y, K, **kw):
    n, D = X.shape
    dev = "cuda"
    coef, intercept = torch.empty(K, D, device=dev, dtype=F64), torch.empty(K, device=dev, dtype=F64)
    info, loss = torch.empty(4, device=dev, dtype=I32), torch.empty(1, device=dev, dtype=F64)
    ws = torch.empty(ops.logreg_workspace_bytes(n, D, K), device=dev, dtype=torch.uint8)
    x, yy = up(X), up(y.astype(np.int32))
    ops.logreg_fit(x, yy, K, ws, coef, intercept, info, loss, **kw)
    dec, pred = torch.empty(n, K, device=dev, dtype=F64), torch.empty(n, device=dev, dtype=I32)
    correct = torch.empty(1, device=dev, dtype=I32)
    ops.logreg_predict(x, yy, coef, intercept, correct, decisions=dec, pred=pred)
    it, fev, status, max_ls = (int(v) for v in info.cpu().numpy())
    return dict(coef=coef.cpu().numpy(), intercept=intercept.cpu().numpy(), n_iter=it, n_fev=fev, status=status,
                max_ls_evals=max_ls, loss=float(loss.item()), decisions=dec.cpu().numpy(), pred=pred.cpu().numpy(),
                correct=int(correct.item()))


CASES = ("main", "conv", "cap", "d1", "rows", "wide", "zero")


def case(gold, name):
    if name == "main":
        return gold["train_points"], gold["train_labels"], {k: gold["main_" + k] for k in ("n_iter", "delta")} | \
            {"decisions": gold["main_train_decisions"]}
    p = f"fit_{name}_"
    return gold[p + "x"].astype(np.float64), gold[p + "y"], {k: gold[p + k] for k in ("n_iter", "delta", "decisions")}


def test_fixture_shapes(gold):
    """The cases the kernel can go wrong at are the ones recorded."""
    shapes = {n: case(gold, n)[0].shape + (case(gold, n)[2]["decisions"].shape[1],) for n in CASES}
    assert shapes["conv"] == (600, 8, 3) and shapes["d1"] == (601, 1, 3) and shapes["rows"] == (1025, 20, 6)
    assert shapes["wide"] == (257, 64, 16) and int(gold["fit_cap_n_iter"]) == 100
    assert not case(gold, "zero")[0][:, -1].any()
    assert max(int(gold[f"fit_{n}_max_ls_evals"]) for n in CASES[1:]) > 1


@pytest.mark.parametrize("name", CASES)
def test_fit_matches_sklearn(ops, gold, name):
    X, y, ref = case(gold, name)
    K = ref["decisions"].shape[1]
    got = device_fit(ops, X, y, K)
    rest = R.fit(X, y, K)
    tol = float(gold["tol_factor"]) * float(ref["delta"])
    err = np.abs(R.centred(got["decisions"]) - R.centred(ref["decisions"])).max()
    err_r = np.abs(R.centred(got["decisions"]) - R.centred(R.decisions(X, rest["coef"], rest["intercept"]))).max()
    print(f"{name}: n_iter {got['n_iter']} (sklearn {int(ref['n_iter'])}), evaluations {got['n_fev']} (restated "
          f"{rest['n_fev']}), status {got['status']}, centred decision error against sklearn {err:.3g}, against the "
          f"restatement {err_r:.3g}, tol_case {tol:.3g}")
    assert got["status"] == rest["status"] and got["status"] != R.LINE_SEARCH
    assert got["n_iter"] == int(ref["n_iter"]) == rest["n_iter"]
    assert got["n_fev"] == rest["n_fev"] and got["max_ls_evals"] == rest["max_ls_evals"]
    s = np.sort(ref["decisions"], axis=1)
    keep = s[:, -1] - s[:, -2] > 2 * tol
    assert (~keep).mean() <= 0.01
    assert np.array_equal(got["pred"][keep], np.argmax(ref["decisions"], axis=1)[keep])
    # the prediction kernel on its own: decisions of the device's parameters, first maximum, count
    z = R.decisions(X, got["coef"], got["intercept"])
    eps = np.finfo(np.float64).eps  # D + 1 <= 65 additions per decision, each within eps of the sum of magnitudes
    assert np.abs(got["decisions"] - z).max() <= 80 * eps * (np.abs(X) @ np.abs(got["coef"]).T +
                                                             np.abs(got["intercept"])).max()
    assert np.array_equal(got["pred"], np.argmax(got["decisions"], axis=1))
    assert got["correct"] == int((got["pred"] == y).sum())
    # the loss returned is the loss at the parameters returned (n <= 1025 terms, each within a few eps)
    w = np.concatenate([got["coef"], got["intercept"][:, None]], 1)
    assert abs(got["loss"] - R.loss_grad(w, X, y, 1.0 / len(y))[0]) <= 1e-12 * max(1.0, abs(got["loss"]))


@pytest.mark.parametrize("name", ["conv", "wide"])
def test_fit_repeats_bitwise(ops, gold, name):
    X, y, ref = case(gold, name)
    K = ref["decisions"].shape[1]
    a, b = device_fit(ops, X, y, K), device_fit(ops, X, y, K)
    for k in ("coef", "intercept", "decisions", "pred"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["n_iter"], a["n_fev"], a["status"], a["loss"]) == (b["n_iter"], b["n_fev"], b["status"], b["loss"])


def test_fit_max_iter_and_ties(ops, gold):
    """max_iter ends the run where the restatement ends it; equal decisions predict the first class."""
    X, y, ref = case(gold, "conv")
    got, rest = device_fit(ops, X, y, 3, max_iter=5), R.fit(X, y, 3, max_iter=5)
    assert (got["n_iter"], got["status"], got["n_fev"]) == (5, R.MAX_ITER, rest["n_fev"])
    dev = "cuda"
    x = torch.zeros(3, 2, device=dev, dtype=F64)
    coef, b = torch.zeros(4, 2, device=dev, dtype=F64), up(np.array([1.0, 2.0, 2.0, 0.5]))
    pred, correct = torch.empty(3, device=dev, dtype=I32), torch.empty(1, device=dev, dtype=I32)
    ops.logreg_predict(x, up(np.array([1, 2, 7], np.int32)), coef, b, correct, pred=pred)
    assert pred.cpu().tolist() == [1, 1, 1] and int(correct.item()) == 1


# ------------------------------------------------------------------ the score
def test_score_matches_reference(M, gold):
    grid = M.FactorGrid(gold["sizes"])
    res = M.beta_vae_score(up(gold["codes"]), grid, seed=int(gold["seed"]), batch_size=int(gold["batch"]),
                           num_train=int(gold["num_train"]), num_eval=int(gold["num_eval"]), return_fit=True)
    left = gold["main_left_out"]
    print(f"score {res['train_accuracy']}, {res['eval_accuracy']}; reference {gold['scores']}; rows left out {left}")
    assert res["n_iter"] == int(gold["main_n_iter"]) and res["status"] == R.CONVERGED_GRAD
    assert abs(res["train_accuracy"] - gold["scores"][0]) <= left[0] / int(gold["num_train"])
    assert abs(res["eval_accuracy"] - gold["scores"][1]) <= left[1] / int(gold["num_eval"])
    assert res["coef"].shape == (3, 6) and res["intercept"].shape == (3,)
    plain = M.beta_vae_score(gold["codes"], grid, seed=int(gold["seed"]), batch_size=int(gold["batch"]),
                             num_train=int(gold["num_train"]), num_eval=int(gold["num_eval"]))
    assert plain == {k: res[k] for k in ("train_accuracy", "eval_accuracy")}


def test_refusals_launch_nothing(M, ops, gold, monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    for name in ("beta_features", "logreg_fit", "logreg_predict"):
        monkeypatch.setattr(ops, name, no_launch)
    with pytest.raises(ValueError, match="at least 3 factors"):
        M.beta_vae_score(np.zeros((12, 4), np.float32), M.FactorGrid([4, 3]))
    with pytest.raises(ValueError, match="at most 16"):
        M.beta_vae_score(np.zeros((2 ** 17, 4), np.float32), M.FactorGrid([2] * 17))
    grid = M.FactorGrid(gold["sizes"])
    with pytest.raises(ValueError, match="never occurs as a label"):
        M.beta_vae_score(gold["codes"], grid, num_train=2, num_eval=5)
    for d in (0, 65):
        with pytest.raises(ValueError, match="1..64"):
            M.beta_vae_score(np.zeros((60, d), np.float32), grid)
    with pytest.raises(ValueError, match="token_pca"):
        M.beta_vae_score(np.zeros((60, 3, 4), np.float32), grid)


def test_score_raises_on_failed_line_search(M, ops, gold, monkeypatch):
    """beta_vae_score turns the fit's status 3 into a RuntimeError that names it, and scores nothing."""
    def failed(x, y, classes, workspace, coef, intercept, info, loss, **kw):
        coef.zero_(), intercept.zero_(), loss.zero_()
        info.copy_(torch.tensor([4, 57, R.LINE_SEARCH, 50], dtype=I32))
    monkeypatch.setattr(ops, "logreg_fit", failed)
    with pytest.raises(RuntimeError, match="line search failed in iteration 4 .after 57 evaluations"):
        M.beta_vae_score(gold["codes"], M.FactorGrid(gold["sizes"]), batch_size=int(gold["batch"]),
                         num_train=int(gold["num_train"]), num_eval=int(gold["num_eval"]))


def test_token_pca_takes_a_misaligned_view(M):
    """A contiguous view that starts 4 bytes into its storage is copied, not refused."""
    tokens = R.make_tokens((257, 3, 16))
    flat = torch.empty(tokens.size + 1, device="cuda", dtype=F32)
    flat[1:] = up(tokens).reshape(-1)
    view = flat[1:].view(257, 3, 16)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got, want = M.token_pca(view), M.token_pca(up(tokens))
    assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_validation_metrics_beta_vae(M, gold, monkeypatch):
    """validation_metrics(beta_vae=True) adds "beta_VAE", spelled as eval_func spells it, with
    beta_vae_score at its defaults (10 000 / 5 000 points of 64 pairs); without the flag the dict is
    the one it has always returned."""
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self, eval_name):  # validation_metrics needs eval_name alone
            object.__setattr__(self, "eval_name", eval_name)

    monkeypatch.setitem(M._NAMED, "stub", [int(v) for v in gold["sizes"]])
    grid = M.FactorGrid.named("stub")
    codes = up(gold["codes"])
    model = Bare("stub")
    plain = model.validation_metrics(codes=codes)
    assert plain == {"factor_VAE": M.factor_vae_score(codes, grid), "MIG": M.mig_score(codes, grid)}
    out = model.validation_metrics(codes=codes, beta_vae=True)
    assert sorted(out) == ["MIG", "beta_VAE", "factor_VAE"] and {k: out[k] for k in plain} == plain
    assert out["beta_VAE"] == M.beta_vae_score(codes, grid, seed=0)
    assert sorted(out["beta_VAE"]) == ["eval_accuracy", "train_accuracy"]
    assert 0.5 < out["beta_VAE"]["eval_accuracy"] <= 1.0
