"""GPU tests of the boosted-tree kernels behind DCI (csrc/gbt.hip) and of metrics.dci_score, against
the numpy restatement tests/gbt_restate.py on the same inputs, and against the reference's own runs
recorded in tests/golden/dci_small.npz (tools/gen_golden_dci.py).

Bounds.  Node tables (feature, threshold bits, row counts): exact -- trees are grown on integer
gradient sums, and the restatement sums the squares behind the impurity in the kernel's order.  Leaf
values and raw predictions: relative 1e-10 with a floor of 1e-12; the two sides differ by the last
bits of exp and of a few hundred fp64 additions (1e-16 each), carried through at most 20 stages.
A leaf value is a quotient mean(G) / mean(p (1 - p)): 256 classes of two or three rows give pure leaves
with values above 100 in the first stage, which push p to e^-13 in the second, where the quotient
turns an error of 1e-16 in the numerator into 1e-10 in the value on either side; that case therefore
runs its single stage, and the 20-stage cases have at most 40 classes.
Importances: absolute 1e-10, they are sums of such terms normalised to 1.  Predictions: equal, every
case being checked on the CPU side to have a gap above 1e-8 between its two largest raw predictions.
Against the reference: mean +- 4 std of its 16 unseeded runs (entries within 1e-9 of the mean count
as equal), as tests/test_dci_host.py holds the restatement to.
"""
import os

import numpy as np
import pytest
import torch

import gbt_restate as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dci_small.npz")
F64, F32, I32 = torch.float64, torch.float32, torch.int32
SCORES = ("informativeness_train", "informativeness_test", "disentanglement", "completeness")


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
def gold():
    return dict(np.load(GOLD))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(y, dims, classes, seed):
    """Column 0 carries the label, column 1 (where there is one) is rounded to steps of 0.25, so it
    holds duplicates, the rest is noise."""
    z = np.random.RandomState(seed).randn(len(y), dims)
    x = 0.5 * z
    x[:, 0] += 2.0 * y / max(classes - 1, 1)
    if dims > 1:
        x[:, 1] = np.round((x[:, 1] + (y % 2)) * 4) / 4
    return x.astype(np.float32)


# name: (num_train, num_test, D, classes, stages)
SHAPES = {
    "n2_d1_c2": (2, 5, 1, 2, 1),
    "n63_d7_c3": (63, 40, 7, 3, 20),
    "n64_d7_c2": (64, 40, 7, 2, 20),
    "n65_d64_c3": (65, 40, 64, 3, 2),
    "n257_d7_c5": (257, 100, 7, 5, 20),
    "n300_d7_c40_absent": (300, 200, 7, 40, 4),
    "n600_d3_c256": (600, 100, 3, 256, 1),  # one stage: see the module docstring on leaf conditioning
    "early_leaf": (100, 50, 2, 2, 3),
    "all_constant": (65, 30, 3, 3, 2),
    "tied_columns": (257, 100, 5, 3, 20),
}
_CASES = {}


def case(name):
    """(x_train, y_train, x_test, y_test, classes, stages) and the restatement's fit, made once."""
    if name in _CASES:
        return _CASES[name]
    n, m, dims, values, stages = SHAPES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "n2_d1_c2":
        y, yt = np.array([0, 1]), rs.randint(2, size=m)
    elif name == "n600_d3_c256":
        y, yt = np.concatenate([np.arange(256), rs.randint(256, size=n - 256)]), rs.randint(256, size=m)
    elif name == "n300_d7_c40_absent":
        allowed = np.array([v for v in range(40) if v not in (7, 23)])
        y, yt = allowed[rs.randint(38, size=n)], rs.randint(40, size=m)
        yt[:2] = (7, 23)
    else:
        y, yt = rs.randint(values, size=n), rs.randint(values, size=m)
    x, xt = table(y, dims, values, 1), table(yt, dims, values, 2)
    if name == "early_leaf":  # column 0 splits the classes cleanly: the root's children are pure
        x[:, 0], xt[:, 0] = y + 0.25 * (x[:, 0] - 2.0 * y).clip(-1, 1), yt
    if name == "n600_d3_c256":  # every column orders the rows by class (column 1 backwards, with duplicates), so
        # the greedy cuts isolate a class's two or three rows and every row has one clear winner
        for a, lab in ((x, y), (xt, yt)):
            a[:, 0], a[:, 1], a[:, 2] = lab + 0.1 * np.tanh(a[:, 0]), -lab, lab + 0.1 * np.tanh(a[:, 2])
    if name == "all_constant":
        x[:], xt[:] = 0.75, 0.75
    if name == "tied_columns":
        x[:, 3], xt[:, 3] = x[:, 0], xt[:, 0]
    classes, ye, yte = R.encode_labels(y, yt)
    ref = R.fit(x, ye, xt, yte, classes, stages, 0.1, tie_seed=5)
    _CASES[name] = (x, ye.astype(np.int32), xt, yte.astype(np.int32), classes, stages, ref)
    return _CASES[name]


def device_fit(ops, x, y, xt, yt, classes, stages, tie_seed=5, learning_rate=0.1):
    """ops.gbt_fit with every output filled with garbage first; all outputs as numpy."""
    (n, dims), m, t = x.shape, xt.shape[0], 1 if classes == 2 else classes
    dx, dxt = up(x), up(xt)
    xs, order = torch.sort(dx.t().contiguous(), dim=1, stable=True)
    ws = torch.full((ops.gbt_workspace_bytes(n, m, dims, classes),), 0xA5, device="cuda", dtype=torch.uint8)
    out = {"raw_train": torch.full((n, t), float("nan"), device="cuda", dtype=F64),
           "raw_test": torch.full((m, t), float("nan"), device="cuda", dtype=F64),
           "pred_train": torch.full((n,), -7, device="cuda", dtype=I32),
           "pred_test": torch.full((m,), -7, device="cuda", dtype=I32),
           "correct": torch.full((2,), -7, device="cuda", dtype=I32),
           "importance": torch.full((dims,), float("nan"), device="cuda", dtype=F64),
           "trees": torch.full((1,), -7, device="cuda", dtype=I32)}
    nodes = (torch.full((stages, t, 15), -9, device="cuda", dtype=I32),
             torch.full((stages, t, 15), float("nan"), device="cuda", dtype=F32),
             torch.full((stages, t, 15), -9, device="cuda", dtype=I32),
             torch.full((stages, t, 15), float("nan"), device="cuda", dtype=F64))
    ops.gbt_fit(dx, xs, order.to(I32), up(y), dxt, up(yt), classes, up(R.init_raw(y.astype(np.int64), classes)), ws,
                out["raw_train"], out["raw_test"], out["pred_train"], out["pred_test"], out["correct"],
                out["importance"], n_estimators=stages, learning_rate=learning_rate, tie_seed=tie_seed,
                trees_used=out["trees"], nodes=nodes)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in zip(("feature", "threshold", "count", "value"), nodes):
        res[k] = v.cpu().numpy()
    return res


def assert_close(out, ref, rel, floor, what):
    err = np.abs(out - ref)
    bound = np.maximum(rel * np.abs(ref), floor)
    print(f"{what}: worst error {err.max():.3e}, worst error / bound {(err / bound).max():.3e}")
    assert np.isfinite(out).all() and (err <= bound).all(), f"{what}: worst error {err.max():.3e}"


def raw_gap(raw, classes):
    if classes == 2:
        return np.abs(raw[:, 0]).min()
    top = np.sort(raw, axis=1)
    return (top[:, -1] - top[:, -2]).min()


@pytest.mark.parametrize("name", list(SHAPES))
def test_fit_against_restatement(ops, name):
    """Node tables exact, leaf values, raw predictions and importances to the stated bounds,
    predictions and accuracy counts equal; a second launch repeats bitwise."""
    x, y, xt, yt, classes, stages, ref = case(name)
    got = device_fit(ops, x, y, xt, yt, classes, stages)
    assert np.array_equal(got["feature"], ref["feature"]), "split features differ"
    assert np.array_equal(got["threshold"].view(np.int32), ref["threshold"].view(np.int32)), "threshold bits differ"
    assert np.array_equal(got["count"], ref["count"]), "node row counts differ"
    assert_close(got["value"], ref["value"], 1e-10, 1e-12, f"{name} leaf values")
    assert_close(got["raw_train"], ref["raw_train"], 1e-10, 1e-12, f"{name} raw_train")
    assert_close(got["raw_test"], ref["raw_test"], 1e-10, 1e-12, f"{name} raw_test")
    assert_close(got["importance"], ref["importance"], 0.0, 1e-10, f"{name} importance")
    assert int(got["trees"][0]) == ref["trees"]
    gap = min(raw_gap(ref["raw_train"], classes), raw_gap(ref["raw_test"], classes))
    assert gap > 1e-8, f"the case's smallest raw gap is {gap:.3e}: choose other inputs"
    assert np.array_equal(got["pred_train"], ref["pred_train"]) and np.array_equal(got["pred_test"], ref["pred_test"])
    assert got["correct"][0] == int(np.sum(ref["pred_train"] == y)) and got["correct"][1] == int(np.sum(ref["pred_test"] == yt))
    again = device_fit(ops, x, y, xt, yt, classes, stages)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), f"{k}: a second launch differs"
    if name == "n600_d3_c256":  # every column orders the rows by class (column 1 backwards, with duplicates), so
        # the greedy cuts isolate a class's two or three rows and every row has one clear winner
        for a, lab in ((x, y), (xt, yt)):
            a[:, 0], a[:, 1], a[:, 2] = lab + 0.1 * np.tanh(a[:, 0]), -lab, lab + 0.1 * np.tanh(a[:, 2])
    if name == "all_constant":
        assert (ref["feature"][:, :, 0] == -1).all() and ref["trees"] == 0 and not got["importance"].any()
    if name == "early_leaf":  # stage 0: the root splits on column 0 and both children are leaves
        assert ref["feature"][0, 0, 0] == 0 and (ref["feature"][0, 0, 1:3] == -1).all()
    if name == "tied_columns":  # both copies win some of their ties
        picked = ref["feature"][ref["feature"] >= 0]
        assert (picked == 0).any() and (picked == 3).any()
    if name == "n300_d7_c40_absent":
        assert classes == 38 and (yt == -1).sum() >= 2


def test_another_tie_seed(ops):
    """tie_seed reaches the hash: another seed gives the restatement's trees for that seed, which
    differ from the first seed's where copies (or other tied cuts) compete."""
    x, y, xt, yt, classes, stages, ref = case("tied_columns")
    other = device_fit(ops, x, y, xt, yt, classes, stages, tie_seed=6)
    ref6 = R.fit(x, y.astype(np.int64), xt, yt.astype(np.int64), classes, stages, 0.1, tie_seed=6)
    assert not np.array_equal(ref6["feature"], ref["feature"])
    assert np.array_equal(other["feature"], ref6["feature"]) and np.array_equal(other["count"], ref6["count"])
    assert np.array_equal(other["threshold"].view(np.int32), ref6["threshold"].view(np.int32))
    assert_close(other["raw_test"], ref6["raw_test"], 1e-10, 1e-12, "raw_test under another tie_seed")


def test_refusals(ops):
    """Sizes outside the limits are refused by the library before anything is launched."""
    from encdiff_amd._lib import HipError
    for args in ((1, 5, 3, 2), (16385, 5, 3, 2), (10, 0, 3, 2), (10, 5, 65, 2), (10, 5, 3, 1), (10, 5, 3, 257)):
        with pytest.raises(HipError, match="ENCDIFF_ERR_SHAPE"):
            ops.gbt_workspace_bytes(*args)


def inside(value, mean, std, what):
    dev = np.abs(np.asarray(value) - mean)
    ok = (dev <= 1e-9) | (dev <= 4 * std)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{what}: worst |x - mean| / std {np.where(dev <= 1e-9, 0, dev / std).max():.2f}")
    assert ok.all(), f"{what}: outside mean +- 4 std of the reference's runs"


def test_dci_score_on_fixture(gold):
    """dci_score end to end on the recorded table: the restatement's scores on the rows the reference
    drew, and inside the reference's own run-to-run band."""
    from encdiff_amd import metrics
    grid = metrics.FactorGrid(gold["sizes"])
    kw = dict(seed=int(gold["seed"]), num_train=int(gold["num_train"]), num_test=int(gold["num_test"]),
              n_estimators=int(gold["n_estimators"]))
    for tie_seed in (0, 3):
        got = metrics.dci_score(torch.from_numpy(gold["main_codes"]).cuda(), grid, tie_seed=tie_seed, **kw)
        ref = R.dci(gold["main_mus_train"].T, gold["main_ys_train"], gold["main_mus_test"].T, gold["main_ys_test"],
                    n_estimators=kw["n_estimators"], tie_seed=tie_seed)
        assert got["importance_matrix"].shape == (7, 4) and got["importance_matrix"].dtype == np.float64
        assert_close(got["importance_matrix"], ref["importance_matrix"], 0.0, 1e-10, "importance matrix")
        for k in SCORES[:2]:
            assert got[k] == ref[k], k
        for k in SCORES[2:]:
            assert abs(got[k] - ref[k]) <= 1e-9, k
        inside(got["importance_matrix"], gold["main_importance_mean"], gold["main_importance_std"], "importance")
        inside([got[k] for k in SCORES], gold["main_scores_mean"], gold["main_scores_std"], "scores")
    again = metrics.dci_score(gold["main_codes"], grid, tie_seed=3, **kw)
    assert again["importance_matrix"].tobytes() == got["importance_matrix"].tobytes()


def test_validation_metrics_dci_key(gold, monkeypatch):
    """validation_metrics(dci=True) adds "dci" with the four scores of dci_score at its defaults;
    without the flag the dict is the one it has always returned."""
    from encdiff_amd import metrics
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self, eval_name):  # validation_metrics needs eval_name alone
            object.__setattr__(self, "eval_name", eval_name)

    monkeypatch.setitem(metrics._NAMED, "stub", [int(v) for v in gold["sizes"]])
    grid = metrics.FactorGrid.named("stub")
    codes = torch.from_numpy(gold["main_codes"]).cuda()
    plain = Bare("stub").validation_metrics(codes=codes, seed=1)
    assert plain == {"factor_VAE": metrics.factor_vae_score(codes, grid, seed=1), "MIG": metrics.mig_score(codes, grid, seed=1)}
    full = Bare("stub").validation_metrics(codes=codes, seed=1, dci=True)
    assert set(full) == {"factor_VAE", "MIG", "dci"} and {k: full[k] for k in plain} == plain
    want = metrics.dci_score(codes, grid, seed=1)
    assert full["dci"] == {k: want[k] for k in SCORES}
    assert 0.5 < full["dci"]["informativeness_test"] <= 1.0
