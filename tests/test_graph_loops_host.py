"""CPU tests of encdiff_amd/graph_loops.py, the host rules every captured sampling loop is built
from: the whole-loop / one-step path policy (through DDIMSampler._path, which reads the patched
module constants at call time), NoiseRows on CPU tensors, and the input rules noise_table and
kernel_mask.  The capture itself and the UNet scope need a device: tests/test_gpu_sampling.py,
test_gpu_inversion.py and test_gpu_ldm.py hold every captured loop against its eager loop."""
import types

import pytest
import torch

from encdiff_amd.graph_loops import NoiseRows, kernel_mask, loop_or_step, noise_table

SHAPE = (2, 3, 4, 4)
S = 3


# ------------------------------------------------------------------ path policy
def expected(after, n):
    return ["step"] * min(after, n) + ["loop"] * max(n - after, 0)


@pytest.mark.parametrize("after", [0, 1, 2])
def test_path_policy_one_key_and_two_interleaved(after, monkeypatch):
    from encdiff_amd.ldm.models.diffusion import ddim as D
    monkeypatch.setattr(D, "LOOP_GRAPH_AFTER", after)
    monkeypatch.setattr(D, "GRAPH_MAX_STEPS", 8)
    s = D.DDIMSampler(types.SimpleNamespace(num_timesteps=1000))
    assert [s._path("a", 8) for _ in range(4)] == expected(after, 4)  # total == GRAPH_MAX_STEPS: a loop graph
    s = D.DDIMSampler(types.SimpleNamespace(num_timesteps=1000))
    got = [(k, s._path(k, 5)) for _ in range(4) for k in ("a", "b")]
    for key in ("a", "b"):  # every key counts its own calls
        assert [kind for k, kind in got if k == key] == expected(after, 4), key


@pytest.mark.parametrize("after", [0, 1, 2])
def test_path_policy_long_loops_replay_the_step_graph_uncounted(after):
    seen = {}
    assert [loop_or_step(seen, "a", 9, after, 8) for _ in range(4)] == ["step"] * 4
    assert seen == {}
    # the same key within the limit afterwards starts counting from its first call
    assert [loop_or_step(seen, "a", 8, after, 8) for _ in range(4)] == expected(after, 4)
    assert seen == {"a": 4}


def test_path_policy_reads_the_constants_at_call_time(monkeypatch):
    from encdiff_amd.ldm.models.diffusion import ddim as D
    s = D.DDIMSampler(types.SimpleNamespace(num_timesteps=1000))
    monkeypatch.setattr(D, "LOOP_GRAPH_AFTER", 0)
    monkeypatch.setattr(D, "GRAPH_MAX_STEPS", 2)
    assert s._path("a", 4) == "step"
    monkeypatch.setattr(D, "GRAPH_MAX_STEPS", 256)
    assert s._path("a", 4) == "loop"
    monkeypatch.setattr(D, "LOOP_GRAPH_AFTER", 5)
    assert s._path("a", 4) == "step"


# ------------------------------------------------------------------ NoiseRows
def table(n):
    g = torch.Generator().manual_seed(3)
    return torch.randn(n, *SHAPE, generator=g)


def test_noise_rows_injected_rows_by_host_index_and_device_counter():
    t = table(S)
    nr = NoiseRows(S, SHAPE, "cpu", injected=True)
    assert nr.table.shape == (S, *SHAPE) and nr.indexed and not nr.draw
    nr.fill(t)
    for i in range(S):
        assert torch.equal(nr.row(i), t[i])
    first = nr.row_at(torch.tensor([0]))
    for i in range(S):
        buf = nr.row_at(torch.tensor([i]))
        assert buf.data_ptr() == first.data_ptr(), "one row buffer: a captured graph holds its address"
        assert buf.shape == SHAPE and torch.equal(buf, t[i])
    assert torch.equal(nr.table, t), "reads leave the injected table as it is"


def test_noise_rows_fill_keeps_the_first_rows_of_a_longer_sequence():
    t = table(S + 2)
    nr = NoiseRows(S, SHAPE, "cpu", injected=True)
    nr.fill(t)
    assert torch.equal(nr.table, t[:S])


def test_noise_rows_drawn_is_one_row_redrawn_on_every_read():
    nr = NoiseRows(S, SHAPE, "cpu", injected=False)
    assert nr.table.shape == (1, *SHAPE) and not nr.indexed and nr.draw
    nr.fill(table(S))  # nothing to inject into: ignored
    assert not nr.table.any()
    torch.manual_seed(0)
    reads = []
    for i in range(S):
        r = nr.row(i)
        assert r.data_ptr() == nr.table.data_ptr() and r.shape == SHAPE
        reads.append(r.clone())
    r = nr.row_at(torch.tensor([1]))
    assert r.data_ptr() == nr.table.data_ptr()
    reads.append(r.clone())
    for a, b in zip(reads, reads[1:]):
        assert not torch.equal(a, b)
    torch.manual_seed(0)
    assert torch.equal(reads[0], torch.randn(SHAPE)), "a read is one N(0, I) draw of the row's shape"


def test_noise_rows_without_draw_stays_zero():
    nr = NoiseRows(S, SHAPE, "cpu", injected=False, draw=False)  # a loop whose sigma is 0
    assert not nr.row(1).any() and not nr.row_at(torch.tensor([2])).any()


# ------------------------------------------------------------------ noise_table, kernel_mask
def test_noise_table_accepts_a_list_and_a_tensor():
    t = table(S + 1).double()
    for seq in (t, list(t)):
        out = noise_table(seq, S, SHAPE, "cpu")
        assert out.dtype == torch.float32 and out.is_contiguous() and torch.equal(out, t.float())


def test_noise_table_refuses_too_few_rows_and_a_wrong_shape():
    with pytest.raises(ValueError, match="normals_sequence must hold 4 draws"):
        noise_table(table(S), S + 1, SHAPE, "cpu")
    with pytest.raises(ValueError, match="mask_normals_sequence must hold 3 draws"):
        noise_table(torch.zeros(S, 2, 3, 4, 5), S, SHAPE, "cpu", "mask_normals_sequence")


def test_kernel_mask():
    B, C, H, W = SHAPE
    img = torch.zeros(SHAPE)
    for shape in ((B, 1, H, W), (B, C, H, W)):
        m = (torch.arange(B * shape[1] * H * W).reshape(shape) % 2).to(torch.float64).transpose(2, 3)
        k = kernel_mask(m, img)
        assert k.dtype == torch.float32 and k.is_contiguous() and k.shape == shape and torch.equal(k, m.float())
    assert kernel_mask(torch.ones(1, 1, H, W), img) is None
    assert kernel_mask(torch.ones(B, H, W), img) is None
    assert kernel_mask([[1.0]], img) is None
