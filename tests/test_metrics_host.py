"""CPU tests of the host half of the disentanglement metrics (encdiff_amd/metrics.py): the factor
grid, the index samplers against the tables the reference drew (tests/golden/metrics_small.npz,
recorded by tools/gen_golden_metrics.py from the reference's own functions), the accuracy arithmetic
and the refusals, all of which happen before anything is launched."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_small.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


def test_fixture_conditions(gold):
    """The margins the recorder checked: every vote's best ratio is clear of the second by >= 1e-4
    (relative), no sqrt(variance) within 1e-3 of the threshold; one dimension is pruned."""
    assert gold["min_rel_gap"] >= 1e-4 and gold["min_thr_dist"] >= 1e-3
    for b in (16, 64):
        assert gold[f"fvae{b}_active"].tolist() == [True] * 6 + [False]
        assert 0.5 < gold[f"fvae{b}_scores"][1] < 1.0  # not trivially 1


@pytest.mark.parametrize("batch", [16, 64])
def test_fvae_samplers_reproduce_reference_tables(gold, M, batch):
    grid = M.FactorGrid(gold["sizes"])
    rs = np.random.RandomState(int(gold["seed"]))
    p = f"fvae{batch}_"
    var_idx = M.sample_variance_indices(grid, rs, gold[p + "var_idx"].shape[0])
    assert var_idx.dtype == np.int32 and np.array_equal(var_idx, gold[p + "var_idx"])
    for part in ("train", "eval"):  # the same RandomState runs on, as in compute_factor_vae
        idx, fac = M.sample_votes(grid, rs, batch, gold[p + part + "_idx"].shape[0])
        assert idx.dtype == np.int32 and fac.dtype == np.int32
        assert np.array_equal(idx, gold[p + part + "_idx"])
        assert np.array_equal(fac, gold[p + part + "_factor"])


@pytest.mark.parametrize("case,m", [("mig_", 500), ("wide15_", 15), ("wide16_", 16), ("wide17_", 17),
                                    ("wide500_", 500)])
def test_mig_sampler_reproduces_reference_tables(gold, M, case, m):
    grid = M.FactorGrid(gold["wide_sizes"] if case.startswith("wide") else gold["sizes"])
    idx, fac = M.sample_mig(grid, np.random.RandomState(int(gold["seed"])), m)
    assert idx.dtype == np.int32 and fac.dtype == np.int32 and fac.shape == (grid.num_factors, m)
    assert np.array_equal(idx, gold[case + "idx"])
    assert np.array_equal(fac, gold[case + "factors"])


def test_named_grids(gold, M):
    s = M.FactorGrid.named("shapes3d")
    assert s.factor_sizes == [10, 10, 10, 8, 4, 15] and s.size == 480000
    assert s.bases.tolist() == [48000, 4800, 480, 60, 15, 1]
    assert s.index([[0, 0, 0, 0, 0, 0], [9, 9, 9, 7, 3, 14], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1],
                    [3, 1, 4, 1, 3, 9]]).tolist() == [0, 479999, 48000, 1, 3 * 48000 + 4800 + 4 * 480 + 60 + 45 + 9]
    m = M.FactorGrid.named("mpi3d")
    assert m.factor_sizes == [6, 6, 2, 3, 3, 40, 40] and m.size == 1036800
    assert m.bases.tolist() == [172800, 28800, 14400, 4800, 1600, 40, 1]
    assert m.index([[0] * 7, [5, 5, 1, 2, 2, 39, 39], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 2]]).tolist() == \
        [0, 1036799, 14400, 42]
    # the reference's own ground truths on recorded factor rows
    for name, g in (("shapes3d", s), ("mpi3d", m)):
        assert g.factor_sizes == gold[name + "_sizes"].tolist()
        assert np.array_equal(g.index(gold[name + "_factors"]), gold[name + "_index"])
    c = M.FactorGrid.named("cars3d")  # the recorder checked that cars3d's lookup is this mixed radix
    assert c.factor_sizes == gold["cars3d_sizes"].tolist() == [4, 24, 183] and c.size == 17568
    assert c.index([[3, 23, 182], [1, 2, 3]]).tolist() == [17567, 24 * 183 + 2 * 183 + 3]


def test_accuracy_arithmetic(gold, M):
    train = np.array([[5, 0, 1, 0], [1, 7, 3, 0], [0, 2, 3, 0]])
    ev = np.array([[2, 1, 0, 0], [0, 3, 2, 0], [1, 0, 1, 0]])
    # classifier = argmax over factors per column = [0, 1, 1, 0] (first maximum on the tie)
    tr, e = M.accuracy_from_votes(train, ev)
    assert tr == (5 + 7 + 3 + 0) * 1. / 22 and e == (2 + 3 + 2 + 0) * 1. / 10
    for b in (16, 64):  # the reference's votes give the reference's accuracies
        tr, e = M.accuracy_from_votes(gold[f"fvae{b}_train_votes"], gold[f"fvae{b}_eval_votes"])
        assert [tr, e] == gold[f"fvae{b}_scores"][:2].tolist()


def test_refusals(gold, M):
    with pytest.raises(ValueError, match="no ground-truth factor grid"):
        M.FactorGrid.named("celeba")
    codes = gold["codes"]
    grid = M.FactorGrid(gold["sizes"])
    with pytest.raises(ValueError, match="num_bins"):
        M.mig_score(codes, grid, num_bins=10)
    with pytest.raises(ValueError, match="V_k <= 256"):
        M.mig_score(np.zeros((600, 3), np.float32), M.FactorGrid([2, 300]))
    with pytest.raises(ValueError, match="120 observations"):
        M.mig_score(codes[:100], grid)
    with pytest.raises(ValueError, match="120 observations"):
        M.factor_vae_score(codes[:100], grid)
    with pytest.raises(ValueError, match="scalar codes"):
        M.factor_vae_score(np.zeros((120, 7, 4), np.float32), grid)
    with pytest.raises(ValueError, match="batch_size"):
        M.factor_vae_score(codes, grid, batch_size=65)
    from encdiff_amd import ops
    with pytest.raises(ValueError, match="V_k <= 256"):
        ops._factor_sizes([4, 257])


def test_validation_metrics_refusals():
    """A model whose eval_name has no grid, or codes of another length, raise before any launch."""
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self, eval_name):  # validation_metrics needs eval_name alone
            object.__setattr__(self, "eval_name", eval_name)

    with pytest.raises(ValueError, match="no ground-truth factor grid"):
        Bare("celeba").validation_metrics(codes=np.zeros((10, 20), np.float32))
    with pytest.raises(ValueError, match="480000 observations"):
        Bare("shapes3d").validation_metrics(codes=np.zeros((1000, 20), np.float32))
    with pytest.raises(ValueError, match="either codes or pool"):
        Bare("shapes3d").validation_metrics()
