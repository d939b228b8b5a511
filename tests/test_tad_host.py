"""CPU tests of the host half of TAD (encdiff_amd/metrics.py: pack_attributes, tad_from_aurocs and
the refusals, all before anything is launched) and of the numpy restatement the GPU tests lean on
(tests/tad_restate.py), against tests/golden/tad_small.npz: inputs and the output of the reference's
own aurocs_search, recorded by tools/gen_golden_tad.py.

Bound of the areas: ten float32 products of magnitude <= 1 summed in order differ from any other
evaluation order by at most about 12 * 2^-24 = 7e-7; 1e-6 absolute.
"""
import math
import os

import numpy as np
import pytest

import tad_restate as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tad_small.npz")
CASES = ["main", "wide", "a64"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def restated(gold):
    """The restatement's areas of every case, computed once."""
    return {c: R.aurocs(gold[c + "_z"], gold[c + "_targ"], gold["t"]) for c in CASES}


def test_fixture_conditions(gold):
    """The margins the recorder checked: nothing within 1e-3 of the 0.75, 0.2 (entropy) and 0.2
    (range) decisions; base rates inside (0, 1); main has a gated column, ties on thresholds above
    the lowest, attributes removed by each filter and two captured."""
    import torch
    assert np.array_equal(gold["t"], torch.arange(0.0, 1.0001, step=0.1).numpy()) and gold["t"].dtype == np.float32
    for c in CASES:
        assert gold[c + "_margin_auroc"] >= 1e-3 and gold[c + "_margin_ent"] >= 1e-3
        assert gold[c + "_margin_range"] >= 1e-3
        rates = R.base_rates(gold[c + "_targ"])
        assert ((rates > 0) & (rates < 1)).all()
    assert gold["main_z"].shape == (1031, 6) and gold["wide_z"].shape == (300, 65) and gold["a64_targ"].shape == (130, 64)
    assert gold["main_gated"] >= 1 and gold["main_ties"] >= 1 and gold["main_removed_by_ent"] >= 1
    assert gold["main_by_auroc"] < 40 and gold["main_captured"] >= 2
    assert gold["main_min_ungated_range"] > 1.0


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_reference(gold, restated, case):
    """Steps 1-5 against the reference's aurocs (its 40 attributes) within 1e-6; base rates exact;
    gated columns exactly 0.5."""
    ref, out = gold[case + "_aurocs"], restated[case]
    assert out.dtype == np.float32 and out.shape == (gold[case + "_targ"].shape[1], ref.shape[1])
    err = np.abs(out[:40].astype(np.float64) - ref).max()
    print(f"{case}: restatement vs reference, worst {err:.3e} (bound 1e-6)")
    assert err <= 1e-6
    assert np.array_equal(R.base_rates(gold[case + "_targ"])[:40], gold[case + "_base_rates"])
    ma, mi = R.column_range(gold[case + "_z"])
    gated = ~((ma - mi) > np.float32(0.2))
    assert gated.sum() == gold[case + "_gated"]
    assert (ref[:, gated] == 0.5).all() and (out[:, gated] == 0.5).all()


def test_tad_from_aurocs_matches_restatement(gold, restated, M):
    """Step 6 of metrics.py (from joint counts) against the restatement's (from the labels) on the
    same float32 areas, every case; on main the captured set is the recorded one."""
    for case in CASES:
        targ = gold[case + "_targ"]
        want = R.tad(restated[case], targ)
        got = M.tad_from_aurocs(restated[case], R.joint_counts(targ), targ.shape[0])
        assert got["attributes_captured"] == want["attributes_captured"] == gold[case + "_captured"]
        assert np.array_equal(got["captured"], want["captured"])
        assert np.array_equal(got["argmax_latent"], want["argmax_latent"])
        assert abs(got["tad_score"] - want["tad_score"]) <= 1e-9
        for k in ("max_auroc", "auroc_diff", "norm_diff", "ent_red_prop"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-9), (case, k)
    main = M.tad_from_aurocs(restated["main"], R.joint_counts(gold["main_targ"]), 1031)
    assert np.nonzero(main["captured"])[0].tolist() == [3, 7]
    assert np.nonzero(main["max_auroc"] >= 0.75)[0].tolist() == [3, 4, 5, 7]   # 4 and 5 share their entropy
    assert main["argmax_latent"][[3, 4, 7]].tolist() == [0, 4, 1]
    # the same from the reference's own areas
    ref = M.tad_from_aurocs(gold["main_aurocs"], R.joint_counts(gold["main_targ"]), 1031)
    assert np.array_equal(ref["captured"], main["captured"]) and abs(ref["tad_score"] - main["tad_score"]) <= 1e-4


def test_tad_by_hand(M):
    """Three attributes over n = 8 rows, four columns, worked out here and not by the restatement.
    Labels a0 = 11110000, a1 = a2 = 11001100: every base rate is 1/2, a0 is independent of the other
    two (every joint cell 2/8 = 1/2 * 1/2: MI = 0), a1 and a2 are equal.
      MI[i][i] = H = 2 * (1/2) ln((1/2) / (1/4)) = ln 2 (cells FF and TT; FT and TF are empty: 0).
      MI[1][2] = ln 2 as well.  ent_red_prop = 1 - (MI_ii - max_other) / MI_ii = [0, 1, 1].
    Areas:            max  argmax  largest other  auroc_diff  norm_diff
      a0 .9 .6 .5 .5   .9     0        .6            .3       1 - .1/.4 = .75
      a1 .5 .8 .7 .5   .8     1        .7            .1       1 - .2/.3 = 1/3
      a2 .6 .5 .5 .7   .7     3        .6            .1       1 - .1/.2 = .5
    At (0.75, 0.2): a0 passes both, a1 fails the entropy filter, a2 both: TAD = 0.3, 1 captured.
    At (0.65, 1.0): all three: TAD = 0.5."""
    au = np.array([[.9, .6, .5, .5], [.5, .8, .7, .5], [.6, .5, .5, .7]])
    joint = np.array([[4, 2, 2], [2, 4, 4], [2, 4, 4]])
    r = M.tad_from_aurocs(au, joint, 8)
    assert r["attributes_captured"] == 1 and r["captured"].tolist() == [True, False, False]
    assert abs(r["tad_score"] - 0.3) <= 1e-12
    assert r["argmax_latent"].tolist() == [0, 1, 3]
    assert np.allclose(r["max_auroc"], [.9, .8, .7], rtol=0, atol=1e-15)
    assert np.allclose(r["auroc_diff"], [.3, .1, .1], rtol=0, atol=1e-12)
    assert np.allclose(r["norm_diff"], [.75, 1 / 3, .5], rtol=0, atol=1e-12)
    assert np.allclose(r["ent_red_prop"], [0, 1, 1], rtol=0, atol=1e-12)
    mi = M.label_mutual_information(joint, 8)
    assert np.allclose(mi, math.log(2) * np.array([[1, 0, 0], [0, 1, 1], [0, 1, 1]]), rtol=0, atol=1e-15)
    r = M.tad_from_aurocs(au, joint, 8, thresh=0.65, ent_red_thresh=1.0)
    assert r["attributes_captured"] == 3 and abs(r["tad_score"] - 0.5) <= 1e-12


def test_pack_attributes(M):
    import torch
    rs = np.random.RandomState(0)
    for a in (1, 40, 64):
        targ = rs.randint(2, size=(37, a))
        targ[0], targ[1] = 0, 1
        want = [sum(int(b) << i for i, b in enumerate(row)) for row in targ]
        for form in (targ, targ.astype(bool), targ.astype(np.float32), torch.from_numpy(targ),
                     torch.from_numpy(targ.astype(np.float32)), torch.from_numpy(targ.astype(bool))):
            w = M.pack_attributes(form)
            assert w.dtype in (np.int64, torch.int64) and tuple(w.shape) == (37,)
            w = w.numpy() if isinstance(w, torch.Tensor) else w
            assert w.view(np.uint64).tolist() == want, (a, type(form))


def test_refusals(gold, M):
    """Every refusal comes before a launch: there is no device here, and a launch attempt would
    raise RuntimeError (no CPU fallback), not ValueError."""
    z, targ = gold["a64_z"], gold["a64_targ"]
    with pytest.raises(ValueError, match=r"\(N, L\)"):
        M.tad_aurocs(z.reshape(130, 3, 1), targ)
    with pytest.raises(ValueError, match="130 rows"):
        M.tad_aurocs(z, targ[:129])
    with pytest.raises(ValueError, match="A <= 64"):
        M.tad_aurocs(z, np.zeros((130, 65), np.uint8))
    with pytest.raises(ValueError, match="A <= 64"):
        M.pack_attributes(np.zeros((4, 65), np.int64))
    bad = targ.astype(np.int64)
    bad[7, 3] = 2
    with pytest.raises(ValueError, match="0 or 1"):
        M.tad_aurocs(z, bad)
    with pytest.raises(ValueError, match="0 or 1"):
        M.tad_score(z, bad.astype(np.float32) * 0.5)
    import torch
    with pytest.raises(ValueError, match="0 or 1"):
        M.pack_attributes(torch.from_numpy(bad))
    from encdiff_amd import ops
    with pytest.raises(ValueError, match="1..64"):
        ops.tad_counts_shape(6, 65)
    with pytest.raises(ValueError, match="1..64"):
        ops.tad_counts_shape(6, 0)


def test_attribute_metrics_refusals(gold):
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self, eval_name):  # the metric entry points need eval_name alone
            object.__setattr__(self, "eval_name", eval_name)

    m = Bare("celeba")
    z, targ = gold["a64_z"], gold["a64_targ"]
    with pytest.raises(ValueError, match="either tokens or pool"):
        m.attribute_metrics(targ)
    with pytest.raises(ValueError, match="either tokens or pool"):
        m.attribute_metrics(targ, tokens=z, pool=z)
    with pytest.raises(ValueError, match="130 rows"):
        m.attribute_metrics(targ[:100], tokens=z.reshape(130, 3, 1))
    with pytest.raises(ValueError, match="0 or 1"):
        m.attribute_metrics(targ * 2, tokens=z)
    # CelebA still has no factor grid: validation_metrics refuses it as before
    with pytest.raises(ValueError, match="no ground-truth factor grid"):
        m.validation_metrics(codes=np.zeros((10, 20), np.float32))
