"""Disentanglement metrics of the validation codes, scored on the device: the FactorVAE score
(evaluation/metrics/factor_vae.py) and the mutual information gap (mig.py, utils.py) that the
reference's eval_func (main_val.py:38-96) logs after every validation epoch.

The reference scores a code table through a "representation function" that is a row lookup
(``pca_rep[x]``) over "observations" that are dataset indices (``Dataset(np.arange(N))``).  Both
metrics therefore reduce to index sampling (host, here), row gathers, variances, histograms and a few
logarithms (csrc/metrics.hip).  The samplers below consume a ``numpy.random.RandomState`` in exactly
the order the reference does, so a seed yields the reference's index tables; only the votes matrices
(K x D integers), the D global variances and the MIG score come back to the host.

CelebA has no factor grid; its models are scored with TAD (celeba_tad.py; ae_utils_exp.py
aurocs_search) from the 40 binary attributes: per (attribute, token column) ROC areas from integer
counts (csrc/tad.hip), then a few hundred numbers of host arithmetic -- the last section below.

Reconstruction quality is scored as recon_metrics.py scores it: SSIM (calculate_ssim, with the
window of create_window) and MSE of decoded images against their inputs, one fused fp64 kernel
(csrc/recon.hip) -- the section after TAD.  LPIPS is not computed.

DCI (evaluation/metrics/dci.py) fits one gradient-boosted classifier per factor: sklearn's default
GradientBoostingClassifier, 100 stages of depth-3 trees, one tree per class.  Those are fitted on the
device (csrc/gbt.hip) from the rows this file samples; the labels, the class prior and the entropies
of the (D, K) importance matrix are host arithmetic -- the section after MIG.

beta-VAE (evaluation/metrics/beta_vae.py) trains sklearn's default LogisticRegression on the mean
|code difference| of row pairs that share one factor.  The feature table, the whole L-BFGS run (one
launch of one workgroup) and the predictions are device work (csrc/beta_vae.hip); only the two
accuracies and the fit's counters come back -- the section after DCI.

eval_func reduces a 3-D token array (N, units, dim) to one column per unit with PCA(n_components=1).
token_pca does that: moments and projection stream the tokens on the device (csrc/token_pca.hip),
the units' dim x dim eigenproblems are host work -- the last section.
"""
from __future__ import annotations

import numpy as np

NUM_BINS = 20           # discretizer.num_bins of eval_func; fixed in the kernel
MIG_BATCH = 16          # compute_mig's batch_size default: num_train is drawn 16 at a time
MAX_FACTOR_VALUES = 256  # joint counts of one factor kept in LDS (csrc/metrics.hip)
MAX_FACTORS = 16
MAX_DIMS = 64

# eval_name -> factor sizes: the grids ddpm_enc.py:122-130 of the reference binds eval_name to.
# cars3d's index (data/ground_truth/cars3d.py) is a lookup built from sklearn's cartesian() of the
# factor ranges, which enumerates them row-major: the lookup is the identity and the index is this
# same mixed radix.
_NAMED = {
    "shapes3d": [10, 10, 10, 8, 4, 15],
    "mpi3d": [6, 6, 2, 3, 3, 40, 40],
    "cars3d": [4, 24, 183],
}


class FactorGrid:
    """Full-grid ground truth in which every factor is latent: observation index
    sum_k f_k * base_k with base_k = prod(sizes) / cumprod(sizes)[k] (row-major mixed radix)."""

    def __init__(self, factor_sizes):
        sizes = [int(v) for v in factor_sizes]
        if not sizes or min(sizes) < 1:
            raise ValueError(f"factor sizes must be positive, got {list(factor_sizes)}")
        self.factor_sizes = sizes
        self.num_factors = len(sizes)
        self.size = int(np.prod(sizes, dtype=np.int64))
        if self.size >= 2 ** 31:
            raise ValueError(f"grid of {self.size} observations: index tables are int32")
        self.bases = self.size // np.cumprod(sizes, dtype=np.int64)

    @classmethod
    def named(cls, eval_name):
        if eval_name not in _NAMED:
            raise ValueError(f"eval_name {eval_name!r} has no ground-truth factor grid "
                             f"(known: {sorted(_NAMED)}); the disentanglement metrics need one")
        return cls(_NAMED[eval_name])

    def sample_factors(self, num, random_state):
        """(num, K) int64: one randint(size_k, size=num) per factor, in factor order."""
        out = np.empty((num, self.num_factors), dtype=np.int64)
        for k, size in enumerate(self.factor_sizes):
            out[:, k] = random_state.randint(size, size=num)
        return out

    def index(self, factors):
        return np.asarray(factors, dtype=np.int64) @ self.bases

    def __repr__(self):
        return f"FactorGrid({self.factor_sizes})"


# ------------------------------------------------------------------ index samplers (host)
def sample_variance_indices(grid, random_state, num_variance_estimate):
    """var_idx int32 (V,): the rows of the global variance estimate (one sample_factors call)."""
    return grid.index(grid.sample_factors(num_variance_estimate, random_state)).astype(np.int32)


def sample_votes(grid, random_state, batch_size, num_points):
    """vote_idx int32 (P, batch) and vote_factor int32 (P,): per vote randint(num_factors), then
    sample_factors(batch_size), then the chosen column set to its row-0 value."""
    idx = np.empty((num_points, batch_size), dtype=np.int32)
    fac = np.empty(num_points, dtype=np.int32)
    for p in range(num_points):
        k = random_state.randint(grid.num_factors)
        f = grid.sample_factors(batch_size, random_state)
        f[:, k] = f[0, k]
        idx[p] = grid.index(f)
        fac[p] = k
    return idx, fac


def sample_mig(grid, random_state, num_train):
    """mig_idx int32 (M,) and mig_factors int32 (K, M): ceil(num_train / 16) draws of 16 (the last
    one shorter), as utils.generate_batch_factor_code does."""
    parts = []
    i = 0
    while i < num_train:
        n = min(num_train - i, MIG_BATCH)
        parts.append(grid.sample_factors(n, random_state))
        i += n
    f = np.concatenate(parts, 0)
    return grid.index(f).astype(np.int32), np.ascontiguousarray(f.T).astype(np.int32)


def accuracy_from_votes(train_votes, eval_votes):
    """(train_accuracy, eval_accuracy): classifier = argmax(train_votes, axis=0); each accuracy is
    the votes under the classifier over all votes (factor_vae.py:77-93)."""
    train_votes, eval_votes = np.asarray(train_votes, np.int64), np.asarray(eval_votes, np.int64)
    classifier = np.argmax(train_votes, axis=0)
    other = np.arange(train_votes.shape[1])
    train = np.sum(train_votes[classifier, other]) * 1. / np.sum(train_votes)
    ev = np.sum(eval_votes[classifier, other]) * 1. / np.sum(eval_votes)
    return float(train), float(ev)


# ------------------------------------------------------------------ checks (host, before any launch)
def _check_codes(codes, grid):
    if codes.ndim != 2:
        raise ValueError(f"codes must be (N, D) scalar codes, got shape {tuple(codes.shape)}; reduce "
                         f"(N, units, dim) tokens with metrics.token_pca, or pass tokens= to validation_metrics")
    n, d = codes.shape
    if n != grid.size:
        raise ValueError(f"{n} code rows but the factor grid {grid.factor_sizes} has {grid.size} observations")
    if not 1 <= d <= MAX_DIMS:
        raise ValueError(f"{d} code dimensions: the metric kernels take 1..{MAX_DIMS}")


def _check_mig(grid, num_bins, dims):
    if num_bins != NUM_BINS:
        raise ValueError(f"num_bins={num_bins}: the histogram kernel is built for {NUM_BINS} bins")
    big = [v for v in grid.factor_sizes if v > MAX_FACTOR_VALUES]
    if big:
        raise ValueError(f"factor sizes {big}: MIG counts at most {MAX_FACTOR_VALUES} values of a factor "
                         f"(V_k <= {MAX_FACTOR_VALUES})")
    if grid.num_factors > MAX_FACTORS:
        raise ValueError(f"{grid.num_factors} factors: MIG takes at most {MAX_FACTORS}")
    if dims < 2:
        raise ValueError("MIG needs at least two code dimensions (the gap between the two largest MI)")


def _device_codes(codes):
    import torch
    if isinstance(codes, np.ndarray):
        codes = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.float32))
    if not codes.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("the disentanglement metrics run on the HIP device; there is no CPU fallback")
        codes = codes.cuda()
    return codes.detach().to(torch.float32).contiguous()


def _up(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------ scores
def factor_vae_score(codes, grid, seed=0, batch_size=64, num_train=10000, num_eval=5000,
                     num_variance_estimate=10000, prune_threshold=0.05):
    """compute_factor_vae of the reference with eval_func's bindings as defaults.  codes: (N, D)
    device tensor (or numpy, uploaded), N == grid.size.  Returns {"train_accuracy", "eval_accuracy",
    "num_active_dims"}; num_active_dims is the length of the mask, i.e. D, as the reference returns
    it, and 0 with both accuracies 0 when no dimension is active."""
    _check_codes(codes, grid)
    if not 2 <= batch_size <= 64:
        raise ValueError(f"batch_size={batch_size}: the vote kernel takes 2..64 rows per point")
    import torch
    from . import ops
    rs = np.random.RandomState(seed)
    var_idx = sample_variance_indices(grid, rs, num_variance_estimate)
    codes = _device_codes(codes)
    dev, (_, D), K = codes.device, codes.shape, grid.num_factors
    gvar = torch.empty(D, device=dev, dtype=torch.float64)
    ops.gather_colvar(codes, _up(var_idx, dev), gvar)
    active = np.sqrt(gvar.cpu().numpy()) >= prune_threshold
    if not active.any():
        return {"train_accuracy": 0., "eval_accuracy": 0., "num_active_dims": 0}
    votes = []
    for num in (num_train, num_eval):
        idx, fac = sample_votes(grid, rs, batch_size, num)
        v = torch.empty(K, D, device=dev, dtype=torch.int32)
        ops.fvae_votes(codes, _up(idx, dev), _up(fac, dev), K, gvar, prune_threshold, v)
        votes.append(v)
    train, ev = accuracy_from_votes(votes[0].cpu().numpy(), votes[1].cpu().numpy())
    return {"train_accuracy": train, "eval_accuracy": ev, "num_active_dims": int(len(active))}


def mig_score(codes, grid, seed=0, num_train=10000, num_bins=NUM_BINS, edge_f64=None):
    """compute_mig of the reference with eval_func's bindings (histogram discretiser, 20 bins).
    Returns {"discrete_mig"}.  edge_f64: evaluate the histogram edges as NumPy 1.x does (float64,
    rounded to float32 at the end) or as NumPy >= 2 does (float32 throughout); the two differ by at
    most an ulp of an edge.  None: as the installed NumPy does, i.e. what the reference's
    np.histogram would give in this environment."""
    _check_codes(codes, grid)
    _check_mig(grid, num_bins, codes.shape[1])
    if edge_f64 is None:
        edge_f64 = int(np.__version__.split(".")[0]) < 2
    import torch
    from . import ops
    idx, fac = sample_mig(grid, np.random.RandomState(seed), num_train)
    codes = _device_codes(codes)
    dev, (_, D), K = codes.device, codes.shape, grid.num_factors
    edges = torch.empty(D, NUM_BINS, device=dev, dtype=torch.float32)
    counts = torch.empty(ops.mig_counts_shape(D, grid.factor_sizes), device=dev, dtype=torch.int32)
    mi = torch.empty(D, K, device=dev, dtype=torch.float64)
    h = torch.empty(K, device=dev, dtype=torch.float64)
    score = torch.empty(1, device=dev, dtype=torch.float64)
    ops.mig_hist(codes, _up(idx, dev), _up(fac, dev), grid.factor_sizes, edges, counts, edge_f64=edge_f64)
    ops.mig_finalize(counts, grid.factor_sizes, idx.shape[0], mi, h, score)
    return {"discrete_mig": float(score.item())}


# ------------------------------------------------------------------ DCI
DCI_MAX_TRAIN = 16384   # sums of 2^32-scaled gradients over the training rows stay in int64 (csrc/gbt.hip)
DCI_MAX_CLASSES = 256
DCI_KEYS = ("informativeness_train", "informativeness_test", "disentanglement", "completeness")


def sample_dci(grid, random_state, num_train, num_test):
    """(train_idx, train_factors, test_idx, test_factors): compute_dci's two calls of
    generate_batch_factor_code on one random state, the training rows first (see sample_mig)."""
    return sample_mig(grid, random_state, num_train) + sample_mig(grid, random_state, num_test)


def dci_labels(y_train, y_test):
    """(C, train labels, test labels) of one factor: the classes are the distinct values of the
    training sample, numbered 0..C-1 in ascending order; a test value outside them becomes -1 and is
    counted as wrong.  ValueError when C is 1 (sklearn refuses a single class) or above 256."""
    values = np.unique(y_train)
    c = int(values.size)
    if c < 2:
        raise ValueError("a factor takes one value in the training sample: the classifier needs at least 2 classes")
    if c > DCI_MAX_CLASSES:
        raise ValueError(f"a factor takes {c} values in the training sample: the tree kernels take C <= "
                         f"{DCI_MAX_CLASSES} classes")
    pos = np.minimum(np.searchsorted(values, y_test), c - 1)
    test = np.where(values[pos] == y_test, pos, -1)
    return c, np.searchsorted(values, y_train).astype(np.int32), test.astype(np.int32)


def dci_init_raw(labels, classes):
    """fp64 (T,): the raw predictions sklearn starts from, those of the class frequencies clipped to
    [eps32, 1 - eps32]: log(p1 / (1 - p1)) for two classes, log(p) - mean(log(p)) otherwise."""
    eps = float(np.finfo(np.float32).eps)
    prior = np.clip(np.bincount(labels, minlength=classes) / float(len(labels)), eps, 1 - eps)
    if classes == 2:
        return np.array([np.log(prior[1] / (1 - prior[1]))])
    lp = np.log(prior)
    return lp - np.mean(lp)


def _entropy(pk, base):
    """scipy.stats.entropy(pk, base=base) along axis 0; restated (normalise, then -sum p log p /
    log base) where scipy is absent."""
    try:
        from scipy.stats import entropy
    except ImportError:
        pk = pk / np.sum(pk, axis=0, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return -np.sum(np.where(pk > 0, pk * np.log(pk), 0.0), axis=0) / np.log(base)
    return entropy(pk, base=base)


def dci_from_importance(importance_matrix):
    """(disentanglement, completeness) of a (D, K) importance matrix, dci.py:105-135: one minus the
    entropy (base K) of every code's row, weighted by the code's share of the total importance, and
    one minus the entropy (base D) of every factor's column, weighted by the factor's share; an
    all-zero matrix is weighted uniformly."""
    im = np.asarray(importance_matrix, np.float64)
    per_code = 1. - _entropy(im.T + 1e-11, im.shape[1])
    per_factor = 1. - _entropy(im + 1e-11, im.shape[0])
    w = np.ones_like(im) if im.sum() == 0. else im
    dis = np.sum(per_code * (w.sum(axis=1) / w.sum()))
    com = np.sum(per_factor * (w.sum(axis=0) / w.sum()))
    return float(dis), float(com)


def _check_dci(num_train, num_test, n_estimators):
    if not 2 <= num_train <= DCI_MAX_TRAIN:
        raise ValueError(f"num_train={num_train}: the tree kernels take 2..{DCI_MAX_TRAIN} training rows")
    if num_test < 1:
        raise ValueError(f"num_test={num_test}: at least one test row")
    if n_estimators < 1:
        raise ValueError(f"n_estimators={n_estimators}: at least one stage")


def dci_score(codes, grid, seed=0, num_train=10000, num_test=5000, n_estimators=100, learning_rate=0.1, tie_seed=0):
    """compute_dci of the reference with eval_func's sizes as defaults.  Returns
    {"informativeness_train", "informativeness_test", "disentanglement", "completeness"} and
    "importance_matrix", a (D, K) float64 numpy array.  The reference builds its classifiers unseeded,
    so its scores vary from run to run with the order in which sklearn visits tied features; here
    the ties are ranked by a hash of (tie_seed, stage, tree, node, feature) and a call repeats."""
    _check_codes(codes, grid)
    _check_dci(num_train, num_test, n_estimators)
    idx_tr, f_tr, idx_te, f_te = sample_dci(grid, np.random.RandomState(seed), num_train, num_test)
    K = grid.num_factors
    labels = [dci_labels(f_tr[k], f_te[k]) for k in range(K)]
    import torch
    from . import ops
    codes = _device_codes(codes)
    dev, D = codes.device, codes.shape[1]
    x_tr = torch.empty(num_train, D, device=dev, dtype=torch.float32)
    x_te = torch.empty(num_test, D, device=dev, dtype=torch.float32)
    ops.gbt_gather(codes, _up(idx_tr, dev), x_tr)
    ops.gbt_gather(codes, _up(idx_te, dev), x_te)
    xs, order = torch.sort(x_tr.t().contiguous(), dim=1, stable=True)
    order = order.to(torch.int32)
    ws = torch.empty(max(ops.gbt_workspace_bytes(num_train, num_test, D, c) for c, _, _ in labels), device=dev,
                     dtype=torch.uint8)
    importance = torch.empty(K, D, device=dev, dtype=torch.float64)
    correct = torch.empty(K, 2, device=dev, dtype=torch.int32)
    pred_tr = torch.empty(num_train, device=dev, dtype=torch.int32)
    pred_te = torch.empty(num_test, device=dev, dtype=torch.int32)
    for k, (c, y_tr, y_te) in enumerate(labels):
        t = 1 if c == 2 else c
        raw_tr = torch.empty(num_train, t, device=dev, dtype=torch.float64)
        raw_te = torch.empty(num_test, t, device=dev, dtype=torch.float64)
        ops.gbt_fit(x_tr, xs, order, _up(y_tr, dev), x_te, _up(y_te, dev), c, _up(dci_init_raw(y_tr, c), dev), ws,
                    raw_tr, raw_te, pred_tr, pred_te, correct[k], importance[k], n_estimators=n_estimators,
                    learning_rate=learning_rate, tie_seed=tie_seed)
    im = np.abs(importance.cpu().numpy().T)
    acc = correct.cpu().numpy().astype(np.float64) / np.array([num_train, num_test], np.float64)
    dis, com = dci_from_importance(im)
    return {"informativeness_train": float(np.mean(acc[:, 0])), "informativeness_test": float(np.mean(acc[:, 1])),
            "disentanglement": dis, "completeness": com, "importance_matrix": im}


# ------------------------------------------------------------------ beta-VAE
def sample_beta_vae(grid, random_state, batch_size, num_points):
    """idx1, idx2 int32 (P, batch) and labels int32 (P,): per point randint(num_factors), then
    sample_factors(batch_size) twice, the chosen column of the second set to the first's
    (beta_vae.py _generate_training_sample; every factor is latent, so the observations draw nothing)."""
    idx1 = np.empty((num_points, batch_size), dtype=np.int32)
    idx2 = np.empty((num_points, batch_size), dtype=np.int32)
    labels = np.empty(num_points, dtype=np.int32)
    for p in range(num_points):
        k = random_state.randint(grid.num_factors)
        f1 = grid.sample_factors(batch_size, random_state)
        f2 = grid.sample_factors(batch_size, random_state)
        f2[:, k] = f1[:, k]
        idx1[p], idx2[p], labels[p] = grid.index(f1), grid.index(f2), k
    return idx1, idx2, labels


def _check_beta_vae(grid, batch_size, num_train, num_eval, C, max_iter, tol):
    if grid.num_factors < 3:
        raise ValueError(f"{grid.num_factors} factors: with two classes sklearn fits a binary objective, which the "
                         f"logistic-regression kernel does not (at least 3 factors)")
    if grid.num_factors > MAX_FACTORS:
        raise ValueError(f"{grid.num_factors} factors: the logistic-regression kernel takes at most {MAX_FACTORS}")
    if not 2 <= batch_size <= 64:
        raise ValueError(f"batch_size={batch_size}: the feature kernel takes 2..64 row pairs per point")
    if not 1 <= num_train <= 2 ** 20 or not 1 <= num_eval < 2 ** 24:
        raise ValueError(f"num_train={num_train}, num_eval={num_eval}: 1..2^20 training and 1..2^24-1 evaluation points")
    if not 1 <= max_iter <= 1000 or not C > 0 or not tol >= 0:
        raise ValueError(f"C={C}, max_iter={max_iter}, tol={tol}: C > 0, 1 <= max_iter <= 1000, tol >= 0")


def beta_vae_score(codes, grid, seed=0, batch_size=64, num_train=10000, num_eval=5000, C=1.0, max_iter=100, tol=1e-4,
                   return_fit=False):
    """compute_beta_vae_sklearn of the reference with eval_func's bindings as defaults: sklearn's
    default LogisticRegression (multinomial, L2 with C, L-BFGS from zero, max_iter, tol) on the
    features mean_b |codes[idx1] - codes[idx2]|.  Returns {"train_accuracy", "eval_accuracy"}; with
    return_fit also "coef" (K, D), "intercept" (K,), "n_iter", "n_fev", "status", "loss".  ValueError
    before any launch: fewer than 3 or more than 16 factors, a factor that never occurs as a training
    label (sklearn would fit fewer classes), D outside 1..64.  RuntimeError when a line search of the
    fit ends without meeting its test (status 3)."""
    _check_codes(codes, grid)
    _check_beta_vae(grid, batch_size, num_train, num_eval, C, max_iter, tol)
    rs = np.random.RandomState(seed)
    train = sample_beta_vae(grid, rs, batch_size, num_train)
    ev = sample_beta_vae(grid, rs, batch_size, num_eval)
    K = grid.num_factors
    missing = np.nonzero(np.bincount(train[2], minlength=K) == 0)[0]
    if missing.size:
        raise ValueError(f"factor {int(missing[0])} never occurs as a label among the {num_train} training points: "
                         f"sklearn would fit {K - missing.size} classes")
    import torch
    from . import ops
    codes = _device_codes(codes)
    dev, D = codes.device, codes.shape[1]
    f64 = dict(device=dev, dtype=torch.float64)
    coef, intercept, loss = torch.empty(K, D, **f64), torch.empty(K, **f64), torch.empty(1, **f64)
    info = torch.empty(4, device=dev, dtype=torch.int32)
    correct = torch.empty(2, 1, device=dev, dtype=torch.int32)
    ws = torch.empty(ops.logreg_workspace_bytes(num_train, D, K), device=dev, dtype=torch.uint8)
    for i, (idx1, idx2, labels) in enumerate((train, ev)):
        x = torch.empty(idx1.shape[0], D, **f64)
        labels = _up(labels, dev)
        ops.beta_features(codes, _up(idx1, dev), _up(idx2, dev), x)
        if i == 0:
            ops.logreg_fit(x, labels, K, ws, coef, intercept, info, loss, C_reg=C, max_iter=max_iter, tol=tol)
        ops.logreg_predict(x, labels, coef, intercept, correct[i])
    n_iter, n_fev, status, _ = (int(v) for v in info.cpu().numpy())
    if status == 3:
        raise RuntimeError(f"the logistic regression's line search failed in iteration {n_iter} (after {n_fev} "
                           f"evaluations): {ops.LOGREG_STATUS[3]}")
    hits = correct.cpu().numpy().reshape(2)
    out = {"train_accuracy": float(hits[0] / np.float64(num_train)), "eval_accuracy": float(hits[1] / np.float64(num_eval))}
    if return_fit:
        out.update(coef=coef.cpu().numpy(), intercept=intercept.cpu().numpy(), n_iter=n_iter, n_fev=n_fev,
                   status=status, loss=float(loss.item()))
    return out


# ------------------------------------------------------------------ token PCA
TOKEN_MAX = 64          # units and numbers per unit (csrc/token_pca.hip)


def pca_sign(v):
    """The component signed as sklearn >= 1.5 signs it (svd_flip(u_based_decision=False)): its entry
    of largest magnitude, the first of equals, is positive."""
    s = np.sign(v[np.argmax(np.abs(v))])
    return v * (s if s != 0 else 1.0)


def token_components(cov):
    """(components (U, d), explained_variance (U,)) float64 from the units' covariances (U, d, d): the
    eigenvector of the largest eigenvalue (np.linalg.eigh), signed by pca_sign."""
    cov = np.asarray(cov, np.float64)
    w, v = np.linalg.eigh(cov)
    comps = np.stack([pca_sign(v[u, :, -1]) for u in range(cov.shape[0])])
    return comps, w[:, -1].copy()


def token_pca(tokens):
    """PCA(n_components=1).fit_transform of every unit of tokens (N, U, d) (device tensor or numpy,
    float32), as eval_func reduces 3-D token arrays: returns (codes (N, U) float32 device tensor,
    components (U, d), mean (U, d), explained_variance (U,)), the last three float64 numpy."""
    shape = tuple(tokens.shape)
    if len(shape) != 3:
        raise ValueError(f"tokens must be (N, units, dim), got shape {shape}")
    n, u, d = shape
    if n < 2:
        raise ValueError(f"{n} token rows: the covariance (ddof = 1) needs at least 2")
    if not (1 <= u <= TOKEN_MAX and 1 <= d <= TOKEN_MAX):
        raise ValueError(f"{u} units of {d} numbers: the token kernels take 1..{TOKEN_MAX} of each")
    import torch
    from . import ops
    tokens = _device_codes(tokens)
    if tokens.data_ptr() % 16:  # a view at an odd offset: the kernels load 16 bytes at a time
        tokens = tokens.clone()
    dev = tokens.device
    mean = torch.empty(u, d, device=dev, dtype=torch.float64)
    cov = torch.empty(u, d, d, device=dev, dtype=torch.float64)
    ws = torch.empty(ops.token_workspace_bytes(n, u, d), device=dev, dtype=torch.uint8)
    ops.token_moments(tokens, ws, mean, cov)
    comps, ev = token_components(cov.cpu().numpy())
    codes = torch.empty(n, u, device=dev, dtype=torch.float32)
    ops.token_project(tokens, mean, _up(comps, dev), codes)
    return codes, comps, mean.cpu().numpy(), ev


# ------------------------------------------------------------------ TAD (CelebA attributes)
TAD_MAX_ATTRS = 64      # one packed label word per row (csrc/tad.hip)


def pack_attributes(targ):
    """(N, A) labels in {0, 1} (bool, int or float; device tensor or numpy) -> one word per row, bit a
    = attribute a, a uint64 stored as int64 (numpy in, numpy out; tensor in, tensor on its device
    out).  ValueError on a value outside {0, 1} or A > 64."""
    shape = tuple(targ.shape)
    if len(shape) != 2 or shape[1] < 1:
        raise ValueError(f"attributes must be (N, A) labels, got shape {shape}")
    if shape[1] > TAD_MAX_ATTRS:
        raise ValueError(f"{shape[1]} attributes: a row's labels are packed into one 64-bit word "
                         f"(A <= {TAD_MAX_ATTRS})")
    if isinstance(targ, np.ndarray):
        if not np.isin(targ, (0, 1)).all():
            raise ValueError("attribute labels must be 0 or 1")
        bits = targ.astype(np.uint64) << np.arange(shape[1], dtype=np.uint64)
        return np.bitwise_or.reduce(bits, axis=1).view(np.int64)
    import torch
    if bool(((targ != 0) & (targ != 1)).any()):
        raise ValueError("attribute labels must be 0 or 1")
    # int64 shifts and sums wrap: bit 63 is the sign bit of the stored word
    return ((targ != 0).to(torch.int64) << torch.arange(shape[1], device=targ.device)).sum(1)


def tad_thresholds():
    """The 11 classifier thresholds of calculate_auroc, from torch as the reference takes them."""
    import torch
    return torch.arange(0.0, 1.0001, step=0.1)


def tad_aurocs(z, targ):
    """aurocs_search of the reference on the device.  z: (N, L) float32, the flattened concept
    tokens; targ: (N, A) labels in {0, 1}.  Returns device tensors {"aurocs" (A, L) float32,
    "base_rates" (A,) float32, "label_joint" (A, A) int32, "col_max" (L,), "col_min" (L,)}.
    ValueError when an attribute is constant (base rate 0 or 1: its ROC divides 0 by 0)."""
    if z.ndim != 2:
        raise ValueError(f"z must be the (N, L) table of flattened tokens, got shape {tuple(z.shape)}")
    if targ.ndim != 2 or targ.shape[0] != z.shape[0]:
        raise ValueError(f"{z.shape[0]} rows of z but attributes of shape {tuple(targ.shape)}")
    if z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError(f"z of shape {tuple(z.shape)} is empty")
    packed = pack_attributes(targ)
    import torch
    from . import ops
    z = _device_codes(z)
    dev, (N, Lc), A = z.device, z.shape, targ.shape[1]
    packed = _up(packed, dev) if isinstance(packed, np.ndarray) else packed.to(dev).contiguous()
    f32 = dict(device=dev, dtype=torch.float32)
    col_max, col_min, thr = torch.empty(Lc, **f32), torch.empty(Lc, **f32), torch.empty(Lc, ops.TAD_THRESHOLDS, **f32)
    counts = torch.empty(ops.tad_counts_shape(Lc, A), device=dev, dtype=torch.int32)
    joint = torch.empty(A, A, device=dev, dtype=torch.int32)
    aurocs = torch.empty(A, Lc, **f32)
    ops.tad_range(z, tad_thresholds().to(dev), col_max, col_min, thr)
    ops.tad_counts(z, packed, A, thr, counts)
    ops.tad_label_joint(packed, A, joint)
    ops.tad_auroc(counts, joint, col_max, col_min, N, aurocs)
    pos = joint.diagonal().cpu().numpy()
    const = np.nonzero((pos == 0) | (pos == N))[0]
    if const.size:
        raise ValueError(f"attribute {int(const[0])} is constant over the {N} rows (base rate "
                         f"{int(pos[const[0]] == N)}): its ROC is undefined")
    # tensor / tensor: one correctly rounded float32 division, as targ.sum(0) / N of the reference
    base = joint.diagonal().to(torch.float32) / torch.full((A,), float(N), **f32)
    return {"aurocs": aurocs, "base_rates": base, "label_joint": joint, "col_max": col_max, "col_min": col_min}


def label_mutual_information(label_joint, n):
    """(A, A) float64: the mutual information (natural log) of every pair of binary labels from their
    joint counts, celeba_tad.py:72-104: the sum over the cells FF, FT, TF, TT of jp * log(jp /
    (pi * pj)), a cell with a zero probability contributing 0."""
    tt = np.asarray(label_joint, np.float64)
    p = np.diag(tt)
    pi, pj = p[:, None], p[None, :]
    cells = ((n - pi - pj + tt, n - pi, n - pj), (pj - tt, n - pi, pj), (pi - tt, pi, n - pj), (tt, pi, pj))
    mi = np.zeros_like(tt)
    for joint, mi_count, mj_count in cells:
        jp, qi, qj = joint / n, np.broadcast_to(mi_count / n, tt.shape), np.broadcast_to(mj_count / n, tt.shape)
        ok = (jp != 0) & (qi != 0) & (qj != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            mi += np.where(ok, jp * np.log(jp / (qi * qj)), 0.0)
    return mi


def tad_from_aurocs(aurocs, label_joint, n, thresh=0.75, ent_red_thresh=0.2):
    """The script half of celeba_tad.py (47-120) in float64 on the host, from aurocs (A, L) and the
    label joint counts over n rows.  Per attribute: max_auroc and argmax_latent over the columns;
    auroc_diff = max_auroc minus the largest other column (the argmax column set to 0); norm_diff =
    1 - the largest other (auroc - 0.5) / (max_auroc - 0.5); ent_red_prop = 1 - (MI[i][i] - max_{j
    != i} MI[i][j]) / MI[i][i].  captured = (max_auroc >= thresh) & (ent_red_prop <= ent_red_thresh);
    tad_score = the sum of auroc_diff over the captured attributes."""
    au = np.array(aurocs, dtype=np.float64)
    A = au.shape[0]
    rows = np.arange(A)
    argmax = np.argmax(au, axis=1)
    max_aur = au[rows, argmax]
    nxt = au.copy()
    nxt[rows, argmax] = 0.0
    diff = max_aur - nxt.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = (au - 0.5) / (max_aur - 0.5)[:, None]
    norm[rows, argmax] = 0.0
    norm_diff = 1.0 - norm.max(axis=1)
    mi = label_mutual_information(label_joint, n)
    others = (mi * (1.0 - np.eye(A))).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent_red_prop = 1.0 - (np.diag(mi) - others) / np.diag(mi)
    captured = (max_aur >= thresh) & (ent_red_prop <= ent_red_thresh)
    return {"tad_score": float(diff[captured].sum()), "attributes_captured": int(captured.sum()),
            "max_auroc": max_aur, "argmax_latent": argmax, "auroc_diff": diff, "norm_diff": norm_diff,
            "ent_red_prop": ent_red_prop, "captured": captured}


def tad_score(z, targ, thresh=0.75, ent_red_thresh=0.2):
    """tad_aurocs, then tad_from_aurocs on its (A, L) areas and joint counts read back."""
    res = tad_aurocs(z, targ)
    return tad_from_aurocs(res["aurocs"].cpu().numpy(), res["label_joint"].cpu().numpy(), int(z.shape[0]),
                           thresh=thresh, ent_red_thresh=ent_red_thresh)


# ------------------------------------------------------------------ reconstruction scores
SSIM_WINDOW = 11        # calculate_ssim's window_size default; fixed in the kernel (csrc/recon.hip)
RECON_LAYOUTS = ("reference", "nchw")


def ssim_window():
    """The 11 x 11 float32 weights of recon_metrics.py's create_window, bit for bit: the 1-D
    Gaussian (sigma 1.5) from Python floats, normalised in float32, and its outer product taken
    with torch's float32 mm.  No exact product of two 1-D passes, and the sum is 0.99999993."""
    import torch
    from math import exp
    sigma = 1.5
    gauss = torch.Tensor([exp(-(x - SSIM_WINDOW // 2) ** 2 / float(2 * sigma ** 2)) for x in range(SSIM_WINDOW)])
    col = (gauss / gauss.sum()).unsqueeze(1)
    return col.mm(col.t()).float().contiguous()


def _recon_pair(a, b):
    import torch
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        raise ValueError("the reconstruction scores take torch tensors")
    if a.ndim != 4 or a.shape != b.shape:
        raise ValueError(f"two (B, Ch, H, W) batches of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    if min(a.shape) < 1 or a.numel() >= 2 ** 31:
        raise ValueError(f"batches of shape {tuple(a.shape)}: every axis >= 1 and fewer than 2^31 elements")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"float32 images expected, got {a.dtype} and {b.dtype}")
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("the reconstruction scores run on the HIP device; there is no CPU fallback")


def ssim(a, b):
    """calculate_ssim(a, b) of the reference on the device: fp64 (B,) device tensor, the mean SSIM
    over Ch, H, W of the float32 (B, Ch, H, W) device tensors a and b (any strides)."""
    _recon_pair(a, b)
    from . import ops
    return ops.ssim_mse(a, b)[0]


def mse(a, b):
    """calculate_mse(a, b) of the reference on the device: fp64 (B,) device tensor."""
    _recon_pair(a, b)
    from . import ops
    return ops.ssim_mse(a, b)[1]


def reconstruction_views(x0, x_recon, layout="reference"):
    """The two (B, Ch, H, W) views recon_metrics.py:89-95 scores, as strides over the tensors given.
    x0: (B, H, W, C) as the data gives it; x_recon: (B, C, H, W) as decode_first_stage gives it.
    layout "reference": the script's call, calculate_ssim(x0, x_recon.permute(0, 2, 3, 1)) -- the
    image rows become SSIM's channels and its window slides over the (width, colour) plane, W x C.
    layout "nchw": the textbook call on (B, C, H, W) planes, x0 permuted instead."""
    if layout not in RECON_LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {RECON_LAYOUTS}")
    if x0.ndim != 4 or x_recon.ndim != 4 or tuple(x_recon.permute(0, 2, 3, 1).shape) != tuple(x0.shape):
        raise ValueError(f"x0 (B, H, W, C) and x_recon (B, C, H, W) expected, got {tuple(x0.shape)} and "
                         f"{tuple(x_recon.shape)}")
    if layout == "reference":
        return x0, x_recon.permute(0, 2, 3, 1)
    return x0.permute(0, 3, 1, 2), x_recon


def reconstruction_scores(x0, x_recon, layout="reference", out_ssim=None, out_mse=None):
    """SSIM and MSE of recon_metrics.py for a batch in [-1, 1]: both tensors mapped through
    (x + 1.) / 2. in float32 inside the kernel and scored in the layout of reconstruction_views.
    Returns fp64 (B,) device tensors (ssim, mse), written into out_ssim / out_mse where given."""
    a, b = reconstruction_views(x0, x_recon, layout)
    _recon_pair(a, b)
    from . import ops
    return ops.ssim_mse(a, b, pre_add=1., pre_mul=0.5, out_ssim=out_ssim, out_mse=out_mse)
