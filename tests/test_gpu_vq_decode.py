"""HIP decode of the VQ first stage (vq.hip lookup kernel + VQDecoderExecutor) vs the as-is torch
module on the same weights, on the device.

Bounds.  Indices: equal to the fp64 argmin wherever the fp64 gap between the best and the
second-best squared distance is >= 1e-4 (fp32 evaluation of a distance of order 10 errs by ~1e-6),
the excluded rows <= 2 % of all.  rows: bf16 rounding of the fp32 conv, rel 2^-8 per element.
Images: rel-L2 <= max(2e-2, 2 x the error of the torch decoder under bf16 autocast), both vs
the fp32 torch decoder on the same input: 2e-2 is the encoder's bound on the same kernels
(test_vq_encoder_hip), the factor 2 allows for bf16 weights as well as bf16 activations.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_REL = 2.0 ** -8
# The rows bound is the rounding of the result alone (half a bf16 ulp is at most 2^-8 relative); it
# leaves nothing for the ~1e-7 by which two fp32 summation orders of the 1x1 conv differ, which
# only matters where the conv's terms (of order 1) cancel to an output near zero.  The inputs are
# drawn from a seed at which no reference element is below 2e-3 in magnitude (of seeds 0-11 on the
# CPU generator: 8 and 11; 11 also has one row with an fp64 gap < 1e-4, which exercises the
# exclusion rule).
LOOKUP_SEED = 11


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import encdiff_amd  # noqa: F401


def first_stage(name="shapes3d", seed=0):
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    torch.manual_seed(seed)
    return instantiate_from_config(model_config(name)["params"]["first_stage_config"]).cuda().eval()


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def rows_of(z):
    """NCHW [B][C][H][W] -> [B*H*W][C]."""
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])


def fp64_argmin_gap(z, E):
    """Per row of z: the fp64 argmin over the codebook (lowest index on ties) and the fp64 gap
    between the best and the second-best squared distance."""
    d = ((rows_of(z).double()[:, None, :] - E.double()[None]) ** 2).sum(-1)
    best2 = torch.topk(d, 2, dim=1, largest=False).values
    return torch.argmin(d, dim=1), best2[:, 1] - best2[:, 0]


def lookup_inputs(n_e, e_dim, B, H, W, dis_dim=20, z_ch=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, e_dim, H, W, generator=g).cuda()
    E = torch.randn(n_e, e_dim, generator=g).cuda()
    s = torch.randn(B, dis_dim, generator=g).cuda()
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(e_dim + dis_dim, z_ch, 1).cuda()
    conv0 = torch.nn.Conv2d(e_dim, z_ch, 1).cuda()  # use_disentangled_concat == False
    return z, E, s, conv, conv0


def conv_ref(conv, q_nchw, s):
    B, _, H, W = q_nchw.shape
    with torch.no_grad():
        return rows_of(conv(torch.cat([q_nchw, s[:, :, None, None].expand(-1, -1, H, W)], 1)))


def assert_rows(rows, ref, z_ch):
    got = rows.float()
    err = (got[:, :z_ch] - ref).abs()
    worst = (err / ref.abs().clamp_min(1e-30)).max().item()
    print(f"rows: worst rel err {worst:.3e} (bound {BF16_REL:.3e})")
    assert (err <= BF16_REL * ref.abs()).all(), worst
    assert (got[:, z_ch:] == 0).all()


@pytest.mark.parametrize("n_e,e_dim", [(2048, 3), (37, 4)])
def test_lookup_op(n_e, e_dim):
    from encdiff_amd import ops
    from encdiff_amd.vq import VQDecoderExecutor
    B, H, W, z_ch = 3, 5, 5, 3
    z, E, s, conv, conv0 = lookup_inputs(n_e, e_dim, B, H, W, seed=LOOKUP_SEED)
    T, Wd, b = VQDecoderExecutor.pack_post_quant(E, conv.weight, conv.bias, e_dim)
    n = B * H * W
    idx = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    zq = torch.full_like(z, float("nan"))
    rows = torch.full((n, 8), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.vq_lookup(z, E, idx=idx, zq=zq, rows=rows, table=T, wd=Wd, bias=b, repr=s)
    want, gap = fp64_argmin_gap(z, E)
    keep = gap >= 1e-4
    excluded = (~keep).sum().item()
    print(f"lookup {n_e}x{e_dim}: {excluded} of {n} rows excluded (fp64 gap < 1e-4)")
    assert excluded <= 0.02 * n
    assert (idx >= 0).all() and (idx < n_e).all()
    assert torch.equal(idx.long()[keep], want[keep])
    zq_ref = E[idx.long()].view(B, H, W, e_dim).permute(0, 3, 1, 2)
    assert torch.equal(zq, zq_ref)
    assert_rows(rows, conv_ref(conv, zq_ref, s), z_ch)
    # quantize == 0: post_quant_conv over z itself
    rows0 = torch.full_like(rows, float("nan"))
    wq = conv.weight.detach()[:, :e_dim, 0, 0].contiguous()
    ops.vq_lookup(z, quantize=False, rows=rows0, wq=wq, wd=Wd, bias=b, repr=s)
    assert_rows(rows0, conv_ref(conv, z, s), z_ch)
    # no representation == an explicit zero tensor, bitwise
    rz, rn = torch.full_like(rows, float("nan")), torch.full_like(rows, float("nan"))
    ops.vq_lookup(z, E, rows=rz, table=T, wd=Wd, bias=b, repr=torch.zeros_like(s))
    ops.vq_lookup(z, E, rows=rn, table=T, wd=Wd, bias=b, repr=None)
    assert torch.equal(rz.view(torch.int16), rn.view(torch.int16))
    # use_disentangled_concat == False: the same kernel with dis_dim = 0
    T0, Wd0, b0 = VQDecoderExecutor.pack_post_quant(E, conv0.weight, conv0.bias, e_dim)
    r0 = torch.full_like(rows, float("nan"))
    ops.vq_lookup(z, E, rows=r0, table=T0, wd=Wd0, bias=b0)
    with torch.no_grad():
        assert_rows(r0, rows_of(conv0(zq_ref)), z_ch)


def test_lookup_tie_goes_to_lowest_index():
    from encdiff_amd import ops
    n_e, e_dim, B, H, W = 2048, 3, 3, 5, 5
    z, E, _, _, _ = lookup_inputs(n_e, e_dim, B, H, W, seed=1)
    picks = {(0, 0, 0): 3, (1, 2, 4): 2040, (2, 4, 4): 1000, (2, 0, 1): 0}
    for j in picks.values():
        E[j + 5] = E[j]
    for (b, y, x), j in picks.items():
        z[b, :, y, x] = E[j]
    idx = torch.full((B * H * W,), -1, device="cuda", dtype=torch.int32)
    ops.vq_lookup(z, E, idx=idx)
    idx = idx.view(B, H, W)
    for (b, y, x), j in picks.items():
        assert idx[b, y, x].item() == j, (b, y, x, j, idx[b, y, x].item())


@pytest.mark.parametrize("n_e,e_dim,B,H", [(37, 4, 64, 32),    # 65536 rows: one lane per row
                                           (3000, 3, 1, 7),    # codebook staged in two chunks
                                           (8192, 8, 2, 4),    # the largest supported codebook
                                           (5, 1, 1, 3)])      # fewer codes than lanes
def test_lookup_other_paths(n_e, e_dim, B, H):
    """The paths the decode shapes do not reach: no lane split at large batches, a codebook larger
    than one LDS chunk (with a tie across the chunk boundary), the shape limits."""
    from encdiff_amd import ops
    z, E, _, _, _ = lookup_inputs(n_e, e_dim, B, H, H, seed=2)
    if n_e == 3000:
        E[2900] = E[10]
        z[0, :, 3, 3] = E[10]
    n = B * H * H
    idx = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    zq = torch.full_like(z, float("nan"))
    ops.vq_lookup(z, E, idx=idx, zq=zq)
    want, gap = fp64_argmin_gap(z, E)
    keep = gap >= 1e-4
    if n_e == 3000:
        assert idx.view(B, H, H)[0, 3, 3].item() == 10
        keep[3 * H + 3] = False  # an exact tie: gap 0, checked above
    excluded = (~keep).sum().item()
    print(f"lookup {n_e}x{e_dim}, {n} rows: {excluded} excluded")
    assert excluded <= 0.02 * n + 1
    assert torch.equal(idx.long()[keep], want[keep])
    assert torch.equal(zq, E[idx.long()].view(B, H, H, e_dim).permute(0, 3, 1, 2))


def test_lookup_rejects_unsupported_shapes():
    from encdiff_amd import ops
    from encdiff_amd._lib import HipError
    z9 = torch.randn(1, 9, 2, 2, device="cuda")
    with pytest.raises(HipError, match="ENCDIFF_ERR_SHAPE"):
        ops.vq_lookup(z9, torch.randn(16, 9, device="cuda"), idx=torch.zeros(4, device="cuda", dtype=torch.int32))
    z3 = torch.randn(1, 3, 2, 2, device="cuda")
    with pytest.raises(HipError, match="ENCDIFF_ERR_SHAPE"):
        ops.vq_lookup(z3, torch.randn(8193, 3, device="cuda"), idx=torch.zeros(4, device="cuda", dtype=torch.int32))
    assert not ops.vq_supported(8193, 3) and not ops.vq_supported(16, 9) and ops.vq_supported(8192, 8)


# ------------------------------------------------------------------ decoder
def torch_decode(fs, z, **kw):
    """The as-is torch path of the same module (executor detached for the call)."""
    dec, fs._hip_decoder = fs._hip_decoder, None
    try:
        with torch.no_grad():
            return fs.decode(z, **kw)
    finally:
        fs._hip_decoder = dec


def image_bound(fs, z, ref, **kw):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        auto = torch_decode(fs, z, **kw).float()
    e = rel_l2(auto, ref)
    return max(2e-2, 2 * e), e


def check_image(fs, z, tag, **kw):
    ref = torch_decode(fs, z, **kw)
    with torch.no_grad():
        out = fs.decode(z, **kw)
    bound, auto = image_bound(fs, z, ref, **kw)
    err = rel_l2(out, ref)
    print(f"{tag}: HIP decode rel-L2 {err:.3e}, torch bf16-autocast decoder {auto:.3e}, bound {bound:.3e}")
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert err <= bound, (err, bound)
    return out


def test_decoder_shapes3d_not_quantized():
    fs = first_stage("shapes3d", seed=0)
    fs.enable_hip(decoder=True)
    g = torch.Generator().manual_seed(5)
    z = torch.randn(2, 3, 16, 16, generator=g).cuda()
    s = torch.randn(2, 20, generator=g).cuda()
    out = check_image(fs, z, "shapes3d B=2 no quantize", force_not_quantize=True, disentangled_repr=s)
    assert out.shape == (2, 3, 64, 64)


def lattice_codebook(g, spacing=0.3):
    """A jittered 16 x 16 x 8 lattice (2048 well-separated entries of dimension 3)."""
    ax = [torch.arange(n, dtype=torch.float32) - (n - 1) / 2 for n in (16, 16, 8)]
    E = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) * spacing
    return E + (torch.rand(E.shape, generator=g) - 0.5) * 0.1 * spacing


def test_full_decode_with_quantize():
    fs = first_stage("shapes3d", seed=1)
    g = torch.Generator().manual_seed(6)
    spacing = 0.3
    E = lattice_codebook(g, spacing)
    with torch.no_grad():
        fs.quantize.embedding.weight.copy_(E.cuda())
    B, H, W = 2, 16, 16
    chosen = torch.randint(0, 2048, (B * H * W,), generator=g)
    noise = (torch.rand(B * H * W, 3, generator=g) - 0.5) * 0.2 * spacing  # |noise| <= spacing / 10 per coordinate
    z = (E[chosen] + noise).view(B, H, W, 3).permute(0, 3, 1, 2).contiguous().cuda()
    s = torch.randn(B, 20, generator=g).cuda()
    want, gap = fp64_argmin_gap(z, fs.quantize.embedding.weight.detach())
    assert gap.min().item() >= 1e-2, gap.min().item()
    assert torch.equal(want.cpu(), chosen)
    fs.enable_hip(decoder=True)
    ex = fs._hip_decoder
    out = check_image(fs, z, "shapes3d B=2 quantize", disentangled_repr=s)
    assert out.shape == (2, 3, 64, 64)
    # the indices the executor's lookup takes on this input
    from encdiff_amd import ops
    idx = torch.full((B * H * W,), -1, device="cuda", dtype=torch.int32)
    ops.vq_lookup(z, ex._packed["vq.codebook"], idx=idx)
    assert torch.equal(idx.long().cpu(), chosen)
    # no representation: zeros, as the torch path
    check_image(fs, z, "shapes3d B=2 quantize, no repr")


def test_decoder_celeba128():
    """32 x 32 latent, 40-dim representation, S = 1024 mid attention."""
    fs = first_stage("celeba128", seed=2)
    fs.enable_hip(decoder=True)
    g = torch.Generator().manual_seed(7)
    z = torch.randn(1, 3, 32, 32, generator=g).cuda()
    s = torch.randn(1, 40, generator=g).cuda()
    out = check_image(fs, z, "celeba128 B=1 no quantize", force_not_quantize=True, disentangled_repr=s)
    assert out.shape == (1, 3, 128, 128)


def test_graph_replay_and_repack():
    fs = first_stage("shapes3d", seed=3)
    fs.enable_hip(decoder=True)
    ex = fs._hip_decoder
    g = torch.Generator().manual_seed(8)
    z = torch.randn(2, 3, 16, 16, generator=g).cuda()
    s = torch.randn(2, 20, generator=g).cuda()
    kw = dict(force_not_quantize=True, disentangled_repr=s)
    with torch.no_grad():
        first = fs.decode(z, **kw)
        assert not ex._graphs, "the first decode at a shape runs eager"
        second = fs.decode(z, **kw)
        assert len(ex._graphs) == 1
        third = fs.decode(z, **kw)
        assert len(ex._graphs) == 1
    assert torch.equal(first, second) and torch.equal(first, third)
    # another input through the same graph
    z2 = torch.randn(2, 3, 16, 16, generator=g).cuda()
    check_image(fs, z2, "replayed graph, new input", **kw)
    assert len(ex._graphs) == 1
    # an in-place parameter change re-packs and drops the graphs
    with torch.no_grad():
        fs.decoder.conv_out.bias.add_(0.5)
    moved = check_image(fs, z, "after conv_out.bias += 0.5", **kw)
    assert not ex._graphs
    assert (moved - first).mean().item() == pytest.approx(0.5, abs=1e-3)


# ------------------------------------------------------------------ routing
@pytest.fixture(scope="module")
def ldm():
    from encdiff_amd.configs import model_config
    from encdiff_amd.ldm.util import instantiate_from_config
    torch.manual_seed(4)
    return instantiate_from_config(model_config("shapes3d")).cuda()


def test_enable_hip_default_leaves_decode_on_torch(ldm):
    fs = ldm.first_stage_model
    fs.enable_hip()
    assert fs._hip_encoder is not None and fs._hip_decoder is None
    z = torch.randn(2, 3, 16, 16, device="cuda")
    with torch.no_grad():
        out = fs.decode(z, force_not_quantize=True)
        ref = fs.decoder(fs.post_quant_conv(torch.cat([z, torch.zeros(2, 20, 16, 16, device="cuda")], 1)))
    # the torch modules themselves (fp32; the library's convs need not repeat bitwise between two
    # calls, the bf16 executor would differ by ~1e-2)
    assert rel_l2(out, ref) < 1e-5
    assert fs._hip_decoder is None


def test_routing_through_ldm(ldm, monkeypatch):
    from encdiff_amd.vq import VQDecoderExecutor
    monkeypatch.setenv("ENCDIFF_VQ_DECODE_HIP", "1")
    ldm.setup_hip_training()
    fs = ldm.first_stage_model
    assert isinstance(fs._hip_decoder, VQDecoderExecutor)
    calls = []
    real = fs._hip_decoder.decode

    def spy(h, force_not_quantize=False, disentangled_repr=None):
        calls.append((tuple(h.shape), force_not_quantize, disentangled_repr is not None))
        return real(h, force_not_quantize=force_not_quantize, disentangled_repr=disentangled_repr)

    monkeypatch.setattr(fs._hip_decoder, "decode", spy)
    z = torch.randn(2, 3, 16, 16, device="cuda")
    a = ldm.decode_first_stage(z)
    b = ldm.decode_first_stage(z, force_not_quantize=True)
    assert calls == [((2, 3, 16, 16), False, False), ((2, 3, 16, 16), True, False)]
    assert a.shape == b.shape == (2, 3, 64, 64)
    # decode_first_stage keeps its 1 / scale_factor multiply
    ref = torch_decode(fs, z / ldm.scale_factor, force_not_quantize=True)
    assert rel_l2(b, ref) <= image_bound(fs, z / ldm.scale_factor, ref, force_not_quantize=True)[0]
    img = (torch.rand(2, 64, 64, 3, device="cuda") * 2 - 1)
    n0 = len(calls)
    with torch.no_grad():
        log = ldm.log_images({"image": img}, N=2, ddim_steps=2, sample_swap=True)
    assert len(calls) > n0
    assert log["inputs"].shape == log["reconstruction"].shape == log["samples"].shape == (2, 3, 64, 64)
    assert log["samples_swapping"].shape == (20 * 2, 3, 64, 64)
    assert log["diffusion_row"].shape[1:] == (2, 3, 64, 64)
    for k, v in log.items():
        assert torch.isfinite(v).all(), k
