"""GPU tests of the token PCA kernels (csrc/token_pca.hip) and of metrics.token_pca against the float64
restatement tests/logreg_restate.py, with sklearn's own float32 error as recorded in
tests/golden/beta_vae_small.npz (tools/gen_golden_beta_vae.py).

Bounds.  Moments: the kernel adds N exact fp64 differences (x - row 0) per mean entry and N products of
two of them per covariance entry; with M = max |x - row 0| a sum of N terms bounded by M^2 carries at
most N eps64 * N M^2, so after the division by N - 1 a covariance entry is within 4 N eps64 M^2 (the
factor 4 covers the rank-one correction, the division and the restatement's own rounding) and a mean
entry within 4 N eps64 M.  Projection: at most the larger of sklearn's own float32 fit_transform
error against the same restatement (recorded) and 2 float32 ulp of the largest |projection| -- the
kernel adds in fp64 and rounds once, so it sits near half an ulp.
"""
import os

import numpy as np
import pytest
import torch

import logreg_restate as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_vae_small.npz")
EPS64 = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def ops():
    from encdiff_amd import ops
    return ops


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_moments(ops, tokens):
    n, u, d = tokens.shape
    t = up(tokens)
    mean = torch.empty(u, d, device="cuda", dtype=torch.float64)
    cov = torch.empty(u, d, d, device="cuda", dtype=torch.float64)
    ws = torch.empty(ops.token_workspace_bytes(n, u, d), device="cuda", dtype=torch.uint8)
    ops.token_moments(t, ws, mean, cov)
    return mean.cpu().numpy(), cov.cpu().numpy()


# the shapes of the fixture, and one whose dim is no multiple of 4 (the scalar load path)
SHAPES = {i: s for i, s in enumerate(R.TOKEN_SHAPES)}
SHAPES["odd"] = (130, 5, 7)


@pytest.mark.parametrize("key", list(SHAPES))
def test_moments(ops, key):
    tokens = R.make_tokens(SHAPES[key])
    n = tokens.shape[0]
    mean, cov = device_moments(ops, tokens)
    ref_mean, ref_cov = R.token_moments(tokens)
    m = float(np.abs(tokens.astype(np.float64) - tokens[0].astype(np.float64)).max())
    e_mean, e_cov = np.abs(mean - ref_mean).max(), np.abs(cov - ref_cov).max()
    print(f"{SHAPES[key]}: mean error {e_mean:.3g} (bound {4 * n * EPS64 * m:.3g}), covariance error {e_cov:.3g} "
          f"(bound {4 * n * EPS64 * m * m:.3g})")
    assert e_mean <= 4 * n * EPS64 * m and e_cov <= 4 * n * EPS64 * m * m
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    again = device_moments(ops, tokens)
    assert np.array_equal(again[0], mean) and np.array_equal(again[1], cov)


@pytest.mark.parametrize("key", list(SHAPES))
def test_projection(M, gold, key):
    tokens = R.make_tokens(SHAPES[key])
    codes, comps, mean, ev = M.token_pca(up(tokens))
    assert codes.is_cuda and codes.dtype == torch.float32 and tuple(codes.shape) == tokens.shape[:2]
    ref, ref_comps, ref_mean, ref_ev = R.token_pca(tokens)
    units = np.arange(tokens.shape[1])
    assert (comps[units, np.argmax(np.abs(comps), axis=1)] > 0).all()      # the sign rule
    # Weyl / Davis-Kahan under the moments' bound E = 4 N eps64 M^2 per entry (|E|_2 <= d E, far below
    # the gap between the top two eigenvalues, about 9 against 0.09)
    n, d = tokens.shape[0], tokens.shape[2]
    m = float(np.abs(tokens.astype(np.float64) - tokens[0].astype(np.float64)).max())
    assert np.abs(ev - ref_ev).max() <= d * 4 * n * EPS64 * m * m
    assert (np.sum(comps * ref_comps, axis=1) > 1 - 1e-12).all()
    got = codes.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    ulp = 2 * float(np.spacing(np.float32(np.abs(ref).max())))
    ref_err = float(gold[f"pca{key}_ref_err"]) if isinstance(key, int) else 0.0
    print(f"{SHAPES[key]}: projection error {err:.3g}, bound max(sklearn's {ref_err:.3g}, 2 ulp {ulp:.3g})")
    assert err <= max(ref_err, ulp)
    if f"pca{key}_codes" in gold:  # sklearn's own output, sign included
        assert np.abs(got - gold[f"pca{key}_codes"]).max() <= ref_err + ulp
    again = M.token_pca(up(tokens))
    assert torch.equal(again[0], codes) and np.array_equal(again[1], comps)


def test_refusals(M):
    with pytest.raises(ValueError, match="at least 2"):
        M.token_pca(np.zeros((1, 1, 2), np.float32))
    with pytest.raises(ValueError, match="1..64"):
        M.token_pca(np.zeros((4, 65, 2), np.float32))
    with pytest.raises(ValueError, match="1..64"):
        M.token_pca(np.zeros((4, 2, 65), np.float32))
    with pytest.raises(ValueError, match="units, dim"):
        M.token_pca(np.zeros((4, 2), np.float32))


def test_validation_metrics_tokens(M, gold, monkeypatch):
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self, eval_name):  # validation_metrics needs eval_name alone
            object.__setattr__(self, "eval_name", eval_name)

    monkeypatch.setitem(M._NAMED, "stub", [int(v) for v in gold["sizes"]])
    codes = gold["codes"][:, :5]  # the constant sixth column would make a unit without a direction
    direction = np.abs(np.random.RandomState(1).randn(5, 8)) + 0.1
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    tokens = up((codes[:, :, None] * direction).astype(np.float32))
    model = Bare("stub")
    projected = M.token_pca(tokens)[0]
    # rank-one tokens: the projection is the centred code up to the float32 rounding of the products
    # (half an ulp each, on weights whose squares sum to 1) and of the result
    centred = codes.astype(np.float64) - codes.astype(np.float64).mean(0)
    assert np.abs(projected.cpu().numpy() - centred).max() <= 8 * np.finfo(np.float32).eps * np.abs(codes).max()
    out = model.validation_metrics(tokens=tokens, beta_vae=True, dci=True)
    assert sorted(out) == ["MIG", "beta_VAE", "dci", "factor_VAE"]
    assert out == model.validation_metrics(codes=projected, beta_vae=True, dci=True)
    with pytest.raises(ValueError, match="exactly one"):
        model.validation_metrics(codes=projected, tokens=tokens)
    with pytest.raises(ValueError, match="60 observations"):
        model.validation_metrics(tokens=tokens[:50])
