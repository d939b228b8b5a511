"""GPU tests of the TAD kernels (csrc/tad.hip) and of the scores built on them
(encdiff_amd/metrics.py, LatentDiffusion.attribute_metrics), against tests/golden/tad_small.npz (the
reference's own aurocs_search, tools/gen_golden_tad.py) and the numpy restatement tests/tad_restate.py.

Bounds.  Column maxima and minima, thresholds, counts and joint counts: exact / bitwise.  Areas:
1e-6 absolute -- ten float32 products of magnitude <= 1 summed in order, against a sum the reference
takes in torch's order (at most about 12 * 2^-24 = 7e-7 apart).  TAD: 1e-4 (at most 40 differences
of areas good to 1e-6).
"""
import os

import numpy as np
import pytest
import torch

import tad_restate as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tad_small.npz")
F32, I32 = torch.float32, torch.int32
CASES = ["main", "wide", "a64"]
TILE, STEP = 32, 512   # columns of a counting workgroup, rows it takes per pass (checked against ops below)


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
    assert (ops.TAD_COL_TILE, ops.TAD_ROW_STEP, ops.TAD_THRESHOLDS, ops.TAD_MAX_ATTRS) == (TILE, STEP, 11, 64)
    return ops


@pytest.fixture(scope="module")
def M():
    from encdiff_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def restated(gold):
    """Per fixture case, once: (ma, mi, thr, counts, joint, aurocs) of the restatement."""
    out = {}
    for c in CASES:
        z, targ = gold[c + "_z"], gold[c + "_targ"]
        ma, mi = R.column_range(z)
        thr = R.thresholds(gold["t"], ma, mi)
        cnt, joint = R.counts(z, targ, thr), R.joint_counts(targ)
        out[c] = (ma, mi, thr, cnt, joint, R.aurocs_from_counts(cnt, np.diag(joint), z.shape[0], ma, mi))
    return out


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def torch_thr(t, ma, mi):
    """t * (ma - mi) + mi as torch evaluates it on the CPU in float32 (LatentClass.__call__)."""
    t, ma, mi = (torch.from_numpy(np.ascontiguousarray(v)) for v in (t, ma, mi))
    return (t[None, :] * (ma - mi)[:, None] + mi[:, None]).numpy()


def run_range(ops, z, t):
    L = z.shape[1]
    outs = []
    dz, dt = up(z), up(t)
    for _ in range(2):  # garbage in the outputs; the second launch repeats bitwise
        ma, mi = torch.full((L,), float("nan"), device="cuda"), torch.full((L,), 7.0, device="cuda")
        thr = torch.full((L, 11), float("nan"), device="cuda")
        ops.tad_range(dz, dt, ma, mi, thr)
        outs.append((ma.cpu().numpy(), mi.cpu().numpy(), thr.cpu().numpy()))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes(), "launches differ"
    return outs[0]


# ------------------------------------------------------------------ range
def _range_case(gold, case):
    if case in CASES:
        return gold[case + "_z"]
    rs = np.random.RandomState(5)
    if case == "n1":
        return rs.randn(1, 70).astype(np.float32)
    if case == "rows":   # several row chunks and column tiles, mixed signs and magnitudes, a constant column
        z = (rs.randn(3001, 131) * np.logspace(-3, 3, 131)).astype(np.float32)
        z[:, 64] = -0.0
        z[:, 65] = np.abs(z[:, 65])
        z[:, 66] = -np.abs(z[:, 66])
        return z
    # "rounding": a column whose (ma - mi) + mi is not ma in float32
    z = rs.rand(97, 3).astype(np.float32)
    z[:, 1] = np.float32(0.5)
    z[11, 1], z[40, 1] = np.float32(1.0), np.float32(-3e-8)
    return z


@pytest.mark.parametrize("case", CASES + ["rounding", "n1", "rows"])
def test_range(gold, ops, case):
    """Column maximum and minimum exact; thr bitwise equal to torch's float32 t * (ma - mi) + mi."""
    z, t = _range_case(gold, case), gold["t"]
    ma, mi, thr = run_range(ops, z, t)
    want_ma, want_mi = z.max(axis=0), z.min(axis=0)
    assert np.array_equal(ma, want_ma) and np.array_equal(mi, want_mi)
    want = torch_thr(t, want_ma, want_mi)
    assert want.dtype == np.float32 and thr.tobytes() == want.tobytes()
    assert np.array_equal(want, R.thresholds(t, want_ma, want_mi))  # the restatement agrees with torch
    if case == "rounding":
        a, b = want_ma[1], want_mi[1]
        assert np.float32(np.float32(a - b) + b) != a, "the case lost its point"
        assert thr[1, 10] != a and thr[1, 0] == b


def test_range_nan(ops, gold):
    """A NaN makes both ends of its column NaN, as torch's max and min do; other columns are untouched."""
    z = np.random.RandomState(6).randn(300, 5).astype(np.float32)
    z[123, 2] = np.nan
    ma, mi, _ = run_range(ops, z, gold["t"])
    keep = [0, 1, 3, 4]
    assert np.isnan(ma[2]) and np.isnan(mi[2])
    assert np.array_equal(ma[keep], z[:, keep].max(0)) and np.array_equal(mi[keep], z[:, keep].min(0))


# ------------------------------------------------------------------ counts
def tie_table(n, L, seed):
    """Multiples of 1/8 clipped to [-2, 2]; where there are >= 2 rows every column gets both ends, so
    its range is 4, thr_0 = -2 and thr_5 = t_5 * 4 - 2 = 0 exactly: ties on the minimum and on
    interior thresholds.  Every fourth column is left continuous."""
    rs = np.random.RandomState(seed)
    z = rs.randn(n, L).astype(np.float32)
    q = np.clip(np.round(z * 8) / 8, -2, 2).astype(np.float32)
    if n >= 2:
        q[rs.randint(n, size=L), np.arange(L)] = 2.0
        lo = rs.randint(n, size=L)
        q[lo, np.arange(L)] = -2.0
        hi_lost = q.max(0) < 2.0   # the minimum landed on the maximum's row
        q[(lo[hi_lost] + 1) % n, np.nonzero(hi_lost)[0]] = 2.0
    keep = np.arange(L) % 4 == 3
    q[:, keep] = z[:, keep]
    return q


def np_counts(z, targ, thr):
    """int64 (L, 11, A + 1) by 11 comparisons and float32 matrix products (exact below 2^24 rows)."""
    n, A = targ.shape
    assert n < 2 ** 24
    lab = np.concatenate([targ, np.ones((n, 1), targ.dtype)], 1).astype(np.float32)
    out = np.empty((z.shape[1], 11, A + 1), np.int64)
    for k in range(11):
        out[:, k, :] = ((z >= thr[None, :, k]).astype(np.float32).T @ lab).astype(np.int64)
    return out


COUNT_SHAPES = [  # (N, L, A)
    (1, 1, 1), (1, 6, 40), (63, 1, 64), (64, TILE - 1, 40), (65, TILE + 1, 64), (63, 6, 1), (64, 6, 64),
    (STEP + 1, TILE + 1, 40), (STEP + 1, 6, 1), (1031, 6, 40), (1031, TILE - 1, 64), (1031, 640, 1),
    (20011, 1, 40), (20011, 6, 64), (20011, TILE + 1, 1), (20011, 640, 40), (20011, 640, 64),
    (27001, 640, 40),   # 20 column tiles -> 52 row chunks of 1024 rows: two passes per workgroup
]


@pytest.mark.parametrize("n,L,A", COUNT_SHAPES)
def test_counts(ops, M, gold, n, L, A):
    """Bitwise the numpy count of the 11 comparisons; garbage in the output shows the zeroing; a
    second launch repeats bitwise."""
    z = tie_table(n, L, n + L)
    targ = (np.random.RandomState(A + n).rand(n, A) < np.linspace(0.1, 0.9, A)).astype(np.uint8)
    ma, mi = z.max(0), z.min(0)
    thr = torch_thr(gold["t"], ma, mi)
    if n >= 2:
        tied = np.arange(L) % 4 != 3
        assert (thr[tied, 0] == -2).all() and (thr[tied, 5] == 0).all() and (z[:, tied] == 0).any()
    want = np_counts(z, targ, thr)
    assert (want[:, 0, A] == n).all()   # thr_0 is the minimum: every row passes
    dz, dthr, packed = up(z), up(thr), up(M.pack_attributes(targ))
    outs = []
    for fill in (-7, 1 << 30):
        c = torch.full(ops.tad_counts_shape(L, A), fill, device="cuda", dtype=I32)
        ops.tad_counts(dz, packed, A, dthr, c)
        outs.append(c.cpu().numpy())
    assert np.array_equal(outs[0], want), f"{np.count_nonzero(outs[0] != want)} of {want.size} counts differ"
    assert np.array_equal(outs[0], outs[1])


def test_counts_ignores_high_bits_and_nan(ops, M, gold):
    """Label bits at and above A are not counted; a NaN passes no threshold."""
    n, L, A = 200, 5, 7
    z = tie_table(n, L, 3)
    targ = (np.random.RandomState(9).rand(n, 64) < 0.5).astype(np.uint8)
    thr = torch_thr(gold["t"], z.max(0), z.min(0))
    z[17, 2] = np.nan
    c = torch.empty(ops.tad_counts_shape(L, A), device="cuda", dtype=I32)
    ops.tad_counts(up(z), up(M.pack_attributes(targ)), A, up(thr), c)
    want = np_counts(z, targ[:, :A], thr)
    assert want[2, 0, A] == n - 1
    assert np.array_equal(c.cpu().numpy(), want)


# ------------------------------------------------------------------ label joint counts
def test_label_joint(ops, M):
    for n in (1, 63, 64, 65, STEP + 1, 1031, 20011):
        for A in (1, 40, 64):
            targ = (np.random.RandomState(n + A).rand(n, A) < np.linspace(0.05, 0.95, A)).astype(np.uint8)
            packed = up(M.pack_attributes(targ))
            outs = []
            for fill in (-3, 12345):
                j = torch.full((A, A), fill, device="cuda", dtype=I32)
                ops.tad_label_joint(packed, A, j)
                outs.append(j.cpu().numpy())
            want = targ.astype(np.int64).T @ targ.astype(np.int64)
            assert np.array_equal(outs[0], want), (n, A)
            assert np.array_equal(outs[0], outs[1]), (n, A)


# ------------------------------------------------------------------ AUROC
def run_auroc(ops, cnt, joint, ma, mi, n):
    L, _, A1 = cnt.shape
    out = torch.full((A1 - 1, L), float("nan"), device="cuda")
    ops.tad_auroc(up(cnt.astype(np.int32)), up(joint.astype(np.int32)), up(ma), up(mi), n, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_auroc(ops, gold, restated, case):
    """From the counts of the fixture inputs (numpy): the reference's areas within 1e-6, for the 24
    attributes of a64 the reference does not reach the restatement's; gated columns exactly 0.5."""
    ma, mi, _, cnt, joint, want = restated[case]
    ref = gold[case + "_aurocs"]
    out = run_auroc(ops, cnt, joint, ma, mi, gold[case + "_z"].shape[0])
    err, err_r = np.abs(out[:40].astype(np.float64) - ref).max(), np.abs(out.astype(np.float64) - want).max()
    print(f"{case}: vs the reference {err:.3e}, vs the restatement {err_r:.3e} (bound 1e-6)")
    assert err <= 1e-6 and err_r <= 1e-6
    gated = ~((ma - mi) > np.float32(0.2))
    assert gated.sum() == gold[case + "_gated"] and (out[:, gated] == 0.5).all()
    assert not (out[:, ~gated] == 0.5).all()


def test_auroc_constant_attribute(ops, gold, restated):
    """P = 0 (and Ng = 0) divide 0 by 0: the attribute's row is NaN where the column is not gated,
    0.5 where it is, and every other row keeps its bits."""
    z, t = gold["main_z"], gold["t"]
    ma, mi, thr, cnt, joint, _ = restated["main"]
    base = run_auroc(ops, cnt, joint, ma, mi, z.shape[0])
    gated = ~((ma - mi) > np.float32(0.2))
    for a, value in ((6, 0), (11, 1)):
        targ = gold["main_targ"].copy()
        targ[:, a] = value
        out = run_auroc(ops, R.counts(z, targ, thr), R.joint_counts(targ), ma, mi, z.shape[0])
        assert np.isnan(out[a, ~gated]).all() and (out[a, gated] == 0.5).all()
        others = np.arange(40) != a
        assert out[others].tobytes() == base[others].tobytes()


# ------------------------------------------------------------------ end to end
def test_tad_aurocs_and_score(M, gold, restated):
    z, targ = gold["main_z"], gold["main_targ"]
    res = M.tad_aurocs(z, targ)
    assert all(v.is_cuda for v in res.values())
    ma, mi, _, _, joint, _ = restated["main"]
    assert np.array_equal(res["col_max"].cpu().numpy(), ma) and np.array_equal(res["col_min"].cpu().numpy(), mi)
    assert np.array_equal(res["label_joint"].cpu().numpy(), joint)
    assert np.array_equal(res["base_rates"].cpu().numpy(), gold["main_base_rates"])
    assert np.abs(res["aurocs"].cpu().numpy().astype(np.float64) - gold["main_aurocs"]).max() <= 1e-6
    want = R.tad(restated["main"][5], targ)
    for form in (z, up(z)):
        got = M.tad_score(form, up(targ) if form is not z else targ)
        assert got["attributes_captured"] == want["attributes_captured"] == 2
        assert np.array_equal(got["captured"], want["captured"])
        assert np.array_equal(got["argmax_latent"], want["argmax_latent"])
        print(f"tad_score {got['tad_score']:.6f}, restatement {want['tad_score']:.6f}")
        assert abs(got["tad_score"] - want["tad_score"]) <= 1e-4
    const = targ.copy()
    const[:, 9] = 1
    with pytest.raises(ValueError, match="attribute 9 is constant"):
        M.tad_aurocs(z, const)


def test_attribute_metrics(gold):
    """(N, latent_unit, context_dim) tokens are flattened unit-major: the same result as the (N, L)
    table; a pool goes through encode_dataset's tokens."""
    from encdiff_amd.ldm.models.diffusion.ddpm_enc import LatentDiffusion

    class Bare(LatentDiffusion):
        def __init__(self, eval_name):
            object.__setattr__(self, "eval_name", eval_name)

    model = Bare("celeba")
    z, targ = gold["main_z"], gold["main_targ"]
    flat = model.attribute_metrics(targ, tokens=up(z))
    toks = model.attribute_metrics(up(targ), tokens=up(z).reshape(1031, 3, 2))
    seen = []
    object.__setattr__(model, "encode_dataset", lambda pool: (seen.append(pool), (None, up(z).reshape(1031, 2, 3)))[1])
    pooled = model.attribute_metrics(targ, pool="the pool")
    assert seen == ["the pool"]
    assert flat["TAD"]["attributes_captured"] == 2 and abs(flat["TAD"]["tad_score"] - 0.4972) < 1e-3
    assert sorted(flat["per_attribute"]) == ["argmax_latent", "auroc_diff", "captured", "ent_red_prop", "max_auroc",
                                             "norm_diff"]
    for other in (toks, pooled):
        assert other["TAD"] == flat["TAD"]
        for k, v in flat["per_attribute"].items():
            assert np.array_equal(other["per_attribute"][k], v), k
    # the thresholds reach the score: without the entropy filter attributes 4 and 5 count too
    loose = model.attribute_metrics(targ, tokens=up(z), thresh=0.75, ent_red_thresh=1.0)
    assert loose["TAD"]["attributes_captured"] == 4 and model.attribute_metrics(
        targ, tokens=up(z), thresh=0.995)["TAD"]["attributes_captured"] == 0


def test_attribute_metrics_celeba128_pool(M):
    """A model_config("celeba128") model (eval_name "celeba", 40 tokens of 16: L = 640) answers
    attribute_metrics from an image pool: the tokens encode_dataset leaves on the device, flattened
    unit-major, scored as tad_score scores them; validation_metrics still refuses the model."""
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    torch.manual_seed(0)
    model = instantiate_from_config(model_config("celeba128")).cuda()
    model.setup_hip_training()
    assert model.eval_name == "celeba"
    g = torch.Generator(device="cuda").manual_seed(3)
    pool = torch.randint(0, 256, (192, 128, 128, 3), device="cuda", dtype=torch.uint8, generator=g)
    attrs = (torch.rand(192, 40, device="cuda", generator=g) < 0.4).to(torch.uint8)
    seen, inner = [], model.encode_dataset
    model.encode_dataset = lambda p, **k: seen.append(inner(p, **k)) or seen[-1]
    try:
        out = model.attribute_metrics(attrs, pool=pool)
    finally:
        del model.encode_dataset
    toks = seen[0][1]
    assert len(seen) == 1 and toks.shape == (192, 40, 16) and toks.is_cuda
    want = M.tad_score(toks.reshape(192, 640), attrs)
    assert out["TAD"] == {"tad_score": want["tad_score"], "attributes_captured": want["attributes_captured"]}
    assert np.array_equal(out["per_attribute"]["max_auroc"], want["max_auroc"])
    assert out["per_attribute"]["max_auroc"].shape == (40,) and np.isfinite(out["per_attribute"]["max_auroc"]).all()
    again = model.attribute_metrics(attrs, tokens=toks)
    assert again["TAD"] == out["TAD"]
    with pytest.raises(ValueError, match="no ground-truth factor grid"):
        model.validation_metrics(codes=seen[0][0])


def test_ops_under_graph_capture(ops, M, gold):
    """The four ops captured into one graph replay to the eager bits (no host read or allocation
    inside the ops), from garbage in every output."""
    from encdiff_amd.graph_loops import capture
    z, targ = gold["wide_z"], gold["wide_targ"]
    n, L = z.shape
    A = targ.shape[1]
    dz, dt, packed = up(z), up(gold["t"]), up(M.pack_attributes(targ))
    ma, mi, thr = torch.empty(L, device="cuda"), torch.empty(L, device="cuda"), torch.empty(L, 11, device="cuda")
    counts = torch.empty(ops.tad_counts_shape(L, A), device="cuda", dtype=I32)
    joint = torch.empty(A, A, device="cuda", dtype=I32)
    au = torch.empty(A, L, device="cuda")
    outs = (ma, mi, thr, counts, joint, au)

    def body():
        ops.tad_range(dz, dt, ma, mi, thr)
        ops.tad_counts(dz, packed, A, thr, counts)
        ops.tad_label_joint(packed, A, joint)
        ops.tad_auroc(counts, joint, ma, mi, n, au)

    body()
    torch.cuda.synchronize()
    eager = [t.clone() for t in outs]
    assert np.abs(au.cpu().numpy().astype(np.float64) - gold["wide_aurocs"]).max() <= 1e-6
    graph = capture(body)
    for _ in range(2):
        for t in (ma, mi, thr, au):
            t.fill_(float("nan"))
        counts.fill_(-1), joint.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a.view(I32) if a.dtype == F32 else a, b.view(I32) if b.dtype == F32 else b)
