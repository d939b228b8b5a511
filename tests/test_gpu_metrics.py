"""GPU tests of the disentanglement-metric kernels (csrc/metrics.hip) and of the scores built on them
(encdiff_amd/metrics.py), against tests/golden/metrics_small.npz: inputs, the index tables the
reference drew and the results of the reference's own functions (tools/gen_golden_metrics.py).

Bounds.  Integers (argmin, votes, bin ids, counts) and the float32 histogram edges: exact / bitwise.
fp64 results of a two-pass variance over at most 1e4 terms: relative 1e-12 against float64 numpy on
the same rows (n * 2^-53 ~ 1e-12 at the worst, typically sqrt(n) * 1e-16).  MI, H and MIG: absolute
1e-9 against the reference's values -- each is a sum of at most a few thousand fp64 terms of
magnitude <= 1, each accurate to a few ulps.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_small.npz")
F64, I32 = torch.float64, torch.int32
THR = 0.05
MIG_CASES = [("mig_", 500), ("wide15_", 15), ("wide16_", 16), ("wide17_", 17), ("wide500_", 500)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def ops():
    from encdiff_amd import ops
    return ops


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand_table(n, d, seed):
    return (np.random.RandomState(seed).randn(n, d) * np.linspace(0.02, 3.0, d)).astype(np.float32)


def var64(rows):
    return np.var(rows.astype(np.float64), axis=-2, ddof=1)


def assert_rel(out, ref, rel, what):
    out, ref = np.asarray(out), np.asarray(ref)
    fin = np.isfinite(ref)
    assert np.array_equal(out[~fin], ref[~fin]), f"{what}: non-finite entries differ"
    err = np.abs(out[fin] - ref[fin])
    worst = (err / np.maximum(np.abs(ref[fin]), 1e-300)).max() if err.size else 0.0
    print(f"{what}: worst relative error {worst:.3e} (bound {rel:.0e})")
    assert (err <= rel * np.abs(ref[fin])).all(), f"{what}: worst relative error {worst:.3e}"


# ------------------------------------------------------------------ gather_colvar
@pytest.mark.parametrize("table", ["fixture7", "rand1", "rand20", "rand64"])
def test_gather_colvar(gold, ops, table):
    """fp64 two-pass ddof = 1 column variance of gathered rows; a second launch repeats bitwise."""
    if table == "fixture7":
        codes, idx_all = gold["codes"], gold["fvae64_var_idx"]
    else:
        d = int(table[4:])
        codes = rand_table(1000, d, d)
        idx_all = np.random.RandomState(d + 1).randint(1000, size=10000).astype(np.int32)
    dc = up(codes)
    sizes = [2, 63, 64, 65, 200] + ([10000] if table == "rand20" else [])
    for n in sizes:
        idx = idx_all[:n]
        out, out2 = (torch.full((codes.shape[1],), float("nan"), device="cuda", dtype=F64) for _ in range(2))
        ops.gather_colvar(dc, up(idx), out)
        ops.gather_colvar(dc, up(idx), out2)
        assert_rel(out.cpu().numpy(), var64(codes[idx]), 1e-12, f"colvar {table} n={n}")
        assert torch.equal(out.view(torch.int64), out2.view(torch.int64)), f"{table} n={n}: launches differ"


# ------------------------------------------------------------------ fvae_votes
def run_votes(ops, dc, idx, fac, K, gvar, want_ratio=True):
    P, D = idx.shape[0], dc.shape[1]
    votes = torch.full((K, D), -7, device="cuda", dtype=I32)  # the op zeroes it
    argmin = torch.full((P,), -9, device="cuda", dtype=I32)
    ratio = torch.full((P, D), float("nan"), device="cuda", dtype=F64) if want_ratio else None
    ops.fvae_votes(dc, up(idx), up(fac), K, gvar, THR, votes, argmin, ratio)
    return votes.cpu().numpy(), argmin.cpu().numpy(), None if ratio is None else ratio.cpu().numpy()


@pytest.mark.parametrize("batch", [16, 64])
def test_fvae_votes_fixture(gold, ops, batch):
    """argmin and votes equal the reference's exactly on its own index tables (train and eval, whole
    and P = 1 / 33 / 299, not multiples of the 32 points of a workgroup at D = 7); ratio per element
    against float64 numpy; the pruned dimension 6 is +inf and shifts nothing to column 6."""
    codes, K = gold["codes"], len(gold["sizes"])
    dc, p = up(codes), f"fvae{batch}_"
    gvar = torch.empty(7, device="cuda", dtype=F64)
    ops.gather_colvar(dc, up(gold[p + "var_idx"]), gvar)
    g = gvar.cpu().numpy()
    active = np.sqrt(g) >= THR
    assert np.array_equal(active, gold[p + "active"]) and not active[6]
    assert_rel(g, gold[p + "global_var"].astype(np.float64), 1e-5, "global variance vs the reference's float32")
    for part in ("train", "eval"):
        idx, fac = gold[p + part + "_idx"], gold[p + part + "_factor"]
        ref_argmin, ref_votes = gold[p + part + "_argmin"], gold[p + part + "_votes"]
        for P in (idx.shape[0], 1, 33, 299 if part == "train" else 199):
            votes, argmin, ratio = run_votes(ops, dc, idx[:P], fac[:P], K, gvar)
            assert np.array_equal(argmin, ref_argmin[:P]), f"{part} P={P}"
            want = np.zeros((K, 7), np.int64)
            np.add.at(want, (fac[:P], ref_argmin[:P]), 1)
            assert np.array_equal(votes, want), f"{part} P={P}"
            if P == idx.shape[0]:
                assert np.array_equal(votes, ref_votes)
            ref_ratio = np.where(active, var64(codes[idx[:P]]) / np.where(active, g, 1.0), np.inf)
            assert np.isposinf(ratio[:, 6]).all()
            assert_rel(ratio, ref_ratio, 1e-12, f"ratio {part} batch={batch} P={P}")
            assert votes[:, 6].sum() == 0 and argmin.max() <= 5


def test_fvae_votes_compaction_shifts_left(gold, ops):
    """With dimension 6 moved to the front the same points vote one column further left than their
    dimension: the argmin is the index in the compacted active list."""
    perm = [6, 0, 1, 2, 3, 4, 5]
    codes, K = np.ascontiguousarray(gold["codes"][:, perm]), len(gold["sizes"])
    dc = up(codes)
    gvar = torch.empty(7, device="cuda", dtype=F64)
    ops.gather_colvar(dc, up(gold["fvae64_var_idx"]), gvar)
    votes, argmin, ratio = run_votes(ops, dc, gold["fvae64_train_idx"], gold["fvae64_train_factor"], K, gvar)
    assert np.isposinf(ratio[:, 0]).all()
    assert np.array_equal(argmin, gold["fvae64_train_argmin"])  # dims 1..6 active -> compacted 0..5
    assert np.array_equal(votes, gold["fvae64_train_votes"])
    assert np.array_equal(np.argmin(ratio, axis=1) - 1, argmin)


@pytest.mark.parametrize("d,batch,P", [(20, 2, 70), (20, 37, 9), (64, 64, 5), (33, 3, 6), (1, 5, 300), (3, 64, 65)])
def test_fvae_votes_other_widths(ops, d, batch, P):
    """The other lane mappings (2, 1, 64 and 16 points per wave) and batch sizes, against float64
    numpy on a random table; the inputs' own float64 ratio gap is asserted first."""
    rs = np.random.RandomState(d * 100 + batch)
    codes, K = rand_table(500, d, d + 5), 5
    idx = rs.randint(500, size=(P, batch)).astype(np.int32)
    fac = rs.randint(K, size=P).astype(np.int32)
    dc = up(codes)
    gvar = torch.empty(d, device="cuda", dtype=F64)
    ops.gather_colvar(dc, up(rs.randint(500, size=300).astype(np.int32)), gvar)
    g = gvar.cpu().numpy()
    active = np.sqrt(g) >= THR
    assert not active[0] and active[1:].all()  # column 0 has std 0.02: pruned
    ref_ratio = np.where(active, var64(codes[idx]) / g, np.inf)
    if active.sum() > 1:
        srt = np.sort(ref_ratio, axis=1)
        assert ((srt[:, 1] - srt[:, 0]) >= 1e-9 * srt[:, 1]).all()
    votes, argmin, ratio = run_votes(ops, dc, idx, fac, K, gvar)
    assert_rel(ratio, ref_ratio, 1e-12, f"ratio d={d} batch={batch}")
    want = np.zeros((K, d), np.int64)
    if active.any():
        want_argmin = np.argmin(ref_ratio[:, active], axis=1)
        np.add.at(want, (fac, want_argmin), 1)
    else:  # d == 1: nothing active, argmin -1 and no vote
        want_argmin = np.full(P, -1)
    assert np.array_equal(argmin, want_argmin)
    assert np.array_equal(votes, want)


# ------------------------------------------------------------------ mig_hist / mig_finalize
def mig_inputs(gold, case):
    wide = case.startswith("wide")
    return gold["wide_codes" if wide else "codes"], [int(v) for v in gold["wide_sizes" if wide else "sizes"]]


def run_hist(ops, codes, idx, fac, sizes, edge_f64=False):
    D, M = codes.shape[1], idx.shape[0]
    edges = torch.full((D, 20), float("nan"), device="cuda")
    bins = torch.full((D, M), -1, device="cuda", dtype=I32)
    counts = torch.full(ops.mig_counts_shape(D, sizes), -5, device="cuda", dtype=I32)  # the op zeroes it
    ops.mig_hist(up(codes), up(idx), up(fac), sizes, edges, counts, bins=bins, edge_f64=edge_f64)
    return edges, bins, counts


def counts_of(bins, fac, sizes):
    D, K = bins.shape[0], len(sizes)
    want = np.zeros((D, K, 20, max(sizes)), np.int64)
    for d in range(D):
        for k in range(K):
            np.add.at(want[d, k], (bins[d] - 1, fac[k]), 1)
    return want


@pytest.mark.parametrize("case,m", MIG_CASES)
def test_mig_hist_and_finalize_fixture(gold, ops, case, m):
    """Edges and bin ids bitwise equal to numpy's through the reference's _histogram_discretize
    (the wide table has a constant column: min == max, and a factor of 183 values), counts exact,
    then MI, H and discrete_mig at 1e-9 of the reference's."""
    codes, sizes = mig_inputs(gold, case)
    idx, fac = gold[case + "idx"], gold[case + "factors"]
    assert idx.shape[0] == m and (not case.startswith("wide") or (max(sizes) == 183 and np.ptp(codes[:, 1]) == 0))
    edges, bins, counts = run_hist(ops, codes, idx, fac, sizes, edge_f64=gold["numpy_major"] < 2)
    assert np.array_equal(edges.cpu().numpy().view(np.int32), gold[case + "edges"].view(np.int32))
    assert np.array_equal(bins.cpu().numpy(), gold[case + "bins"])
    assert bins.min().item() >= 1 and bins.max().item() <= 20
    assert np.array_equal(counts.cpu().numpy(), counts_of(gold[case + "bins"], fac, sizes))
    D, K = codes.shape[1], len(sizes)
    mi = torch.full((D, K), float("nan"), device="cuda", dtype=F64)
    h = torch.full((K,), float("nan"), device="cuda", dtype=F64)
    score = torch.full((1,), float("nan"), device="cuda", dtype=F64)
    ops.mig_finalize(counts, sizes, m, mi, h, score)
    for name, out, ref in (("MI", mi, gold[case + "mi"]), ("H", h, gold[case + "h"]),
                           ("discrete_mig", score, gold[case + "score"])):
        err = np.abs(out.cpu().numpy() - ref).max()
        print(f"{case}{name}: max abs error {err:.3e} (bound 1e-09)")
        assert err <= 1e-9, f"{case}{name}: {err:.3e}"


def test_mig_hist_many_chunks(gold, ops):
    """M = 2500 rows (three row chunks of a workgroup) against numpy's own histogram and digitize."""
    codes, sizes = mig_inputs(gold, "wide")
    rs = np.random.RandomState(11)
    f = np.stack([rs.randint(s, size=2500) for s in sizes]).astype(np.int32)
    idx = (f[0] * 183 + f[1]).astype(np.int32)
    x = codes[idx].T
    want_edges = np.stack([np.histogram(r, 20)[1][:-1] for r in x])
    want_bins = np.stack([np.digitize(r, e) for r, e in zip(x, want_edges)])
    edges, bins, counts = run_hist(ops, codes, idx, f, sizes, edge_f64=int(np.__version__.split(".")[0]) < 2)
    assert np.array_equal(edges.cpu().numpy().view(np.int32), want_edges.astype(np.float32).view(np.int32))
    assert np.array_equal(bins.cpu().numpy(), want_bins)
    assert np.array_equal(counts.cpu().numpy(), counts_of(want_bins, f, sizes))
    assert counts.sum().item() == 2500 * 3 * 2


def test_mig_hist_float64_edges(gold, ops):
    """edge_f64: step = (fp64(max) - fp64(min)) / 20, edge_i = fp32(fp64(i) * step + fp64(min)),
    product and sum rounded separately (NumPy 1.x's linspace), restated in float64 numpy."""
    for case in ("mig_", "wide500_"):
        codes, sizes = mig_inputs(gold, case)
        idx, fac = gold[case + "idx"], gold[case + "factors"]
        x = codes[idx].T.astype(np.float64)
        lo, hi = x.min(1), x.max(1)
        lo, hi = np.where(lo == hi, lo - 0.5, lo), np.where(lo == hi, hi + 0.5, hi)
        step = (hi - lo) / 20
        want = (np.arange(20, dtype=np.float64)[None] * step[:, None] + lo[:, None]).astype(np.float32)
        edges, bins, _ = run_hist(ops, codes, idx, fac, sizes, edge_f64=True)
        assert np.array_equal(edges.cpu().numpy().view(np.int32), want.view(np.int32))
        want_bins = np.stack([np.digitize(r, e) for r, e in zip(codes[idx].T, want)])
        assert np.array_equal(bins.cpu().numpy(), want_bins)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("batch", [16, 64])
def test_factor_vae_score_from_seed(gold, batch):
    from encdiff_amd import metrics
    grid = metrics.FactorGrid(gold["sizes"])
    ref = gold[f"fvae{batch}_scores"]
    for codes in (up(gold["codes"]), gold["codes"]):  # device tensor, and numpy (uploaded)
        out = metrics.factor_vae_score(codes, grid, seed=int(gold["seed"]), batch_size=batch, num_train=300,
                                       num_eval=200, num_variance_estimate=200)
        assert out == {"train_accuracy": ref[0], "eval_accuracy": ref[1], "num_active_dims": int(ref[2])}, (out, ref)


def test_factor_vae_score_nothing_active(gold):
    from encdiff_amd import metrics
    out = metrics.factor_vae_score(up(gold["codes"] * 1e-3), metrics.FactorGrid(gold["sizes"]), num_train=10,
                                   num_eval=10, num_variance_estimate=50)
    assert out == {"train_accuracy": 0., "eval_accuracy": 0., "num_active_dims": 0}


@pytest.mark.parametrize("case,m", MIG_CASES)
def test_mig_score_from_seed(gold, case, m):
    from encdiff_amd import metrics
    codes, sizes = mig_inputs(gold, case)
    out = metrics.mig_score(up(codes), metrics.FactorGrid(sizes), seed=int(gold["seed"]), num_train=m,
                            edge_f64=gold["numpy_major"] < 2)  # the NumPy generation that recorded the fixture
    assert list(out) == ["discrete_mig"]
    err = abs(out["discrete_mig"] - float(gold[case + "score"]))
    print(f"{case}: discrete_mig {out['discrete_mig']:.12f}, abs error {err:.3e} (bound 1e-09)")
    assert err <= 1e-9


@pytest.fixture(scope="module")
def model():
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    torch.manual_seed(0)
    m = instantiate_from_config(model_config("shapes3d")).cuda()
    m.setup_hip_training()
    return m


def test_validation_metrics_shapes3d(model):
    """A model built with eval_name = "shapes3d" scores a random (480000, 20) device table at the
    reference's sizes."""
    assert model.eval_name == "shapes3d"
    g = torch.Generator(device="cuda").manual_seed(0)
    codes = torch.randn(480000, 20, device="cuda", generator=g)
    out = model.validation_metrics(codes=codes)
    assert list(out) == ["factor_VAE", "MIG"]
    fv, mig = out["factor_VAE"], out["MIG"]
    assert fv["num_active_dims"] == 20
    assert all(np.isfinite(v) for v in (fv["train_accuracy"], fv["eval_accuracy"], mig["discrete_mig"]))
    assert 0. <= fv["eval_accuracy"] <= 1. and 0. <= fv["train_accuracy"] <= 1. and mig["discrete_mig"] >= 0.


def test_validation_metrics_pool(model):
    """With a pool the images go through encode_dataset and its codes are scored: the same
    dictionary as scoring those codes directly (Cars3D's grid, 17568 images, the smallest named)."""
    g = torch.Generator(device="cuda").manual_seed(1)
    pool = torch.randint(0, 256, (17568, 64, 64, 3), device="cuda", dtype=torch.uint8, generator=g)
    seen, inner = [], model.encode_dataset
    model.eval_name = "cars3d"
    model.encode_dataset = lambda p, **k: seen.append(inner(p, **k)) or seen[-1]
    try:
        out = model.validation_metrics(pool=pool)
        with pytest.raises(ValueError, match="17568 observations"):
            model.validation_metrics(pool=pool[:100])
        assert len(seen) == 1 and seen[0][0].shape == (17568, 20) and seen[0][0].is_cuda
        assert out == model.validation_metrics(codes=seen[0][0])
    finally:
        del model.encode_dataset
        model.eval_name = "shapes3d"
    assert np.isfinite(out["MIG"]["discrete_mig"]) and out["factor_VAE"]["num_active_dims"] in (0, 20)


def test_ops_under_graph_capture(gold, ops):
    """The four ops captured into one graph replay to the eager votes, MI and score (no host read or
    allocation inside the ops)."""
    from encdiff_amd.graph_loops import capture
    codes, sizes = gold["codes"], [int(v) for v in gold["sizes"]]
    dc, K, D = up(codes), len(sizes), 7
    var_idx, vidx, vfac = up(gold["fvae64_var_idx"]), up(gold["fvae64_train_idx"]), up(gold["fvae64_train_factor"])
    midx, mfac = up(gold["mig_idx"]), up(gold["mig_factors"])
    gvar = torch.empty(D, device="cuda", dtype=F64)
    votes = torch.empty(K, D, device="cuda", dtype=I32)
    edges = torch.empty(D, 20, device="cuda")
    counts = torch.empty(ops.mig_counts_shape(D, sizes), device="cuda", dtype=I32)
    mi = torch.empty(D, K, device="cuda", dtype=F64)
    h = torch.empty(K, device="cuda", dtype=F64)
    score = torch.empty(1, device="cuda", dtype=F64)

    def body():
        ops.gather_colvar(dc, var_idx, gvar)
        ops.fvae_votes(dc, vidx, vfac, K, gvar, THR, votes)
        ops.mig_hist(dc, midx, mfac, sizes, edges, counts)
        ops.mig_finalize(counts, sizes, midx.numel(), mi, h, score)

    body()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (gvar, votes, counts, mi, h, score)]
    assert np.array_equal(eager[1].cpu().numpy(), gold["fvae64_train_votes"])
    graph = capture(body)
    for _ in range(2):
        for t in (gvar, mi, h, score):
            t.fill_(float("nan"))
        votes.fill_(-1), counts.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip((gvar, votes, counts, mi, h, score), eager):
            assert torch.equal(a, b)
