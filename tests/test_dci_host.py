"""CPU tests of DCI: the numpy restatement of the boosted trees (tests/gbt_restate.py) against the
reference's own runs recorded in tests/golden/dci_small.npz (tools/gen_golden_dci.py), and the host
half of metrics.dci_score (sampler, labels, refusals, final arithmetic).

Bounds.  Training raw predictions: absolute 1e-9 against sklearn's decision_function -- sums of at
most 20 leaf values of magnitude O(1); the 2^-32 quantisation of the gradients chooses splits and does
not enter the values.  The wide case is left out of that comparison alone: sklearn's own training
predictions differ by O(1) between its 16 runs there (wide_raw_spread; the recorder explains why),
so there is nothing to reproduce, and its training accuracy is held to the band like the other scores.
What sklearn leaves to chance (importances, disentanglement, completeness, test accuracy): inside
mean +- 4 std of the 16 recorded runs, an entry within 1e-9 of the mean counting as equal.
Final arithmetic: 1e-12 against the reference's scores from its own importance matrix.
"""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gbt_restate as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "dci_small.npz")
SCORES = ("informativeness_train", "informativeness_test", "disentanglement", "completeness")
CASES = ("main_", "bin_", "wide_")
_RUNS = {}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def restated(gold, case, tie_seed):
    key = (case, tie_seed)
    if key not in _RUNS:
        with np.errstate(divide="ignore", invalid="ignore"):
            _RUNS[key] = R.dci(gold[case + "mus_train"].T, gold[case + "ys_train"], gold[case + "mus_test"].T,
                               gold[case + "ys_test"], n_estimators=int(gold["n_estimators"]), tie_seed=tie_seed)
    return _RUNS[key]


def inside(value, mean, std, what):
    value = np.asarray(value, np.float64)
    dev = np.abs(value - mean)
    same = (dev <= 1e-9) | (np.isnan(value) & np.isnan(mean))  # one factor: entropy to base 1 is NaN on both sides
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(same, 0.0, dev / std)
    print(f"{what}: worst |x - mean| / std {ratio.max():.2f}")
    assert (same | (dev <= 4 * std)).all(), f"{what}: {ratio.max():.2f} std from the mean of the reference's runs"


@pytest.mark.parametrize("case", ["main_", "bin_"])
@pytest.mark.parametrize("tie_seed", [0, 1, 2, 3])
def test_training_predictions_match_sklearn(gold, case, tie_seed):
    assert gold[case + "raw_spread"] <= 1e-12  # the reference's 16 runs agree: there is one answer
    res = restated(gold, case, tie_seed)
    for i, fit in enumerate(res["fits"]):
        err = np.abs(fit["raw_train"] - gold[f"{case}raw_train{i}"]).max()
        print(f"{case} factor {i}: worst raw_train error {err:.3e}")
        assert err <= 1e-9
        assert fit["acc_train"] == gold[case + "acc_train_max"][i] == gold[case + "acc_train_min"][i]
    assert abs(res["informativeness_train"] - gold[case + "scores_mean"][0]) <= 1e-12


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tie_seed", [0, 1, 2, 3])
def test_chance_scores_inside_reference_band(gold, case, tie_seed):
    res = restated(gold, case, tie_seed)
    inside(res["importance_matrix"], gold[case + "importance_mean"], gold[case + "importance_std"], "importance")
    inside([f["acc_test"] for f in res["fits"]], gold[case + "acc_test_mean"], gold[case + "acc_test_std"], "acc_test")
    inside([f["acc_train"] for f in res["fits"]], gold[case + "acc_train_mean"], gold[case + "acc_train_std"], "acc_train")
    inside([res[k] for k in SCORES], gold[case + "scores_mean"], gold[case + "scores_std"], "scores")


def test_wide_case_has_absent_classes(gold):
    classes, y, yt = R.encode_labels(gold["wide_ys_train"][0], gold["wide_ys_test"][0])
    assert classes == 38 and (yt == -1).sum() >= 2 and gold["wide_raw_spread"] > 1e-3


def test_tie_priority_is_splitmix64():
    """The counter-based hash, against values worked out by hand from the published constants."""
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF  # the first output of splitmix64 seeded with 0
    a, b = R.tie_priority(0, 1, 2, 3, 4), R.tie_priority(0, 1, 2, 3, 5)
    assert a != b and a == R.tie_priority(0, 1, 2, 3, 4) and 0 <= a < 2 ** 64
    assert R.tie_priority(1, 1, 2, 3, 4) != a


def test_sampler_draws_the_reference_tables(gold):
    from encdiff_amd import metrics
    grid = metrics.FactorGrid(gold["sizes"])
    rs = np.random.RandomState(int(gold["seed"]))
    idx_tr, f_tr, idx_te, f_te = metrics.sample_dci(grid, rs, int(gold["num_train"]), int(gold["num_test"]))
    assert np.array_equal(idx_tr, gold["main_train_idx"]) and np.array_equal(idx_te, gold["main_test_idx"])
    assert np.array_equal(f_tr, gold["main_ys_train"]) and np.array_equal(f_te, gold["main_ys_test"])
    assert np.array_equal(gold["main_codes"][idx_tr], gold["main_mus_train"].T)


def test_labels_and_prior(gold):
    from encdiff_amd import metrics
    y, yt = gold["wide_ys_train"][0], gold["wide_ys_test"][0]
    c, a, b = metrics.dci_labels(y, yt)
    rc, ra, rb = R.encode_labels(y, yt)
    assert c == rc == 38 and np.array_equal(a, ra) and np.array_equal(b, rb) and a.dtype == b.dtype == np.int32
    assert set(yt[b == -1]) == {7, 23}
    for classes, labels in ((c, a), (2, gold["bin_ys_train"][0])):
        assert np.array_equal(metrics.dci_init_raw(labels, classes), R.init_raw(labels.astype(np.int64), classes))
    assert metrics.dci_init_raw(np.array([0, 1, 1, 1]), 2)[0] == np.log(0.75 / 0.25)
    with pytest.raises(ValueError, match="one value"):
        metrics.dci_labels(np.full(10, 3), np.arange(10))
    with pytest.raises(ValueError, match="C <= 256"):
        metrics.dci_labels(np.arange(257), np.arange(10))


def test_dci_score_refusals():
    """N, D, C and C == 1 are refused on the host, before the device is touched."""
    from encdiff_amd import metrics
    grid = metrics.FactorGrid([4, 3, 5, 2])
    codes = np.zeros((120, 7), np.float32)
    for kw, match in ((dict(num_train=1), "training rows"), (dict(num_train=16385), "training rows"),
                      (dict(num_test=0), "test row"), (dict(n_estimators=0), "stage")):
        with pytest.raises(ValueError, match=match):
            metrics.dci_score(codes, grid, **kw)
    with pytest.raises(ValueError, match="1..64"):
        metrics.dci_score(np.zeros((120, 65), np.float32), grid)
    with pytest.raises(ValueError, match="scalar codes"):
        metrics.dci_score(np.zeros((120, 7, 2), np.float32), grid)
    with pytest.raises(ValueError, match="one value"):
        metrics.dci_score(np.zeros((8, 3), np.float32), metrics.FactorGrid([1, 8]), num_train=50, num_test=10)
    with pytest.raises(ValueError, match="C <= 256"):
        metrics.dci_score(np.zeros((600, 3), np.float32), metrics.FactorGrid([300, 2]), num_train=5000, num_test=10)


@pytest.mark.parametrize("case", CASES)
def test_final_arithmetic(gold, case):
    """disentanglement and completeness from the reference's importance matrix of one run."""
    from encdiff_amd import metrics
    im, want = gold[case + "importance_run0"], gold[case + "scores_run0"]
    with np.errstate(divide="ignore", invalid="ignore"):
        dis, com = metrics.dci_from_importance(im)
        rdis, rcom = R.scores_from_importance(im)
    for got, ref in ((dis, want[2]), (com, want[3]), (rdis, want[2]), (rcom, want[3])):
        assert (np.isnan(got) and np.isnan(ref)) or abs(got - ref) <= 1e-12


def test_final_arithmetic_all_zero_guard():
    from encdiff_amd import metrics
    dis, com = metrics.dci_from_importance(np.zeros((5, 3)))
    assert abs(dis) <= 1e-12 and abs(com) <= 1e-12  # uniform rows and columns: entropy 1 everywhere
    dis, com = metrics.dci_from_importance(np.eye(3))
    assert abs(dis - 1) <= 1e-8 and abs(com - 1) <= 1e-8


def test_validation_metrics_flag_defaults_off():
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion
    assert inspect.signature(LatentDiffusion.validation_metrics).parameters["dci"].default is False


def test_gbt_args_layout_matches_c():
    """The ctypes mirror of EncdiffGbtArgs has the C layout, and the limits agree with the header."""
    import encdiff_amd._lib as L
    from encdiff_amd import metrics
    hdr = os.path.join(REPO, "include", "encdiff_hip.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', "int main(void){",
             'printf("size %zu\\n", sizeof(EncdiffGbtArgs));',
             'printf("limits %d %d\\n", ENCDIFF_GBT_MAX_TRAIN, ENCDIFF_GBT_MAX_CLASSES);']
    for name, _ in L.GbtArgs._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(EncdiffGbtArgs, {name}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    for line in out.strip().splitlines():
        name, *vals = line.split()
        if name == "size":
            assert C.sizeof(L.GbtArgs) == int(vals[0])
        elif name == "limits":
            assert (metrics.DCI_MAX_TRAIN, metrics.DCI_MAX_CLASSES) == (int(vals[0]), int(vals[1]))
        else:
            assert getattr(L.GbtArgs, name).offset == int(vals[0]), name
