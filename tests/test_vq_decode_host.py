"""CPU tests of the VQ decode head's host side: the ctypes mirror of EncdiffVqArgs has the C
layout (gcc probe against include/encdiff_hip.h), and the pack step that composes
post_quant_conv into a per-code table reproduces the conv."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "encdiff_hip.h")


def test_vq_args_layout_matches_c():
    import encdiff_amd._lib as L
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){",
             'printf("size %zu\\n", sizeof(EncdiffVqArgs));']
    for fname, _ in L.VqArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(EncdiffVqArgs, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        field, val = line.split()
        if field == "size":
            assert C.sizeof(L.VqArgs) == int(val)
        else:
            assert getattr(L.VqArgs, field).offset == int(val), field
            seen += 1
    assert seen == len(L.VqArgs._fields_)
    assert "encdiff_vq_lookup" in L.EXPORTS


@pytest.mark.parametrize("dis_dim", [0, 20])
def test_pack_post_quant_reproduces_conv(dis_dim):
    """T[idx] + Wd s + b == post_quant_conv(cat(E[idx], s)) on CPU fp32, with and without the concat."""
    from encdiff_amd.vq import VQDecoderExecutor
    torch.manual_seed(0)
    n_e, e_dim, z_ch, rows = 2048, 3, 3, 257
    E = torch.randn(n_e, e_dim)
    conv = torch.nn.Conv2d(e_dim + dis_dim, z_ch, 1)
    T, Wd, b = VQDecoderExecutor.pack_post_quant(E, conv.weight, conv.bias, e_dim)
    assert T.shape == (n_e, z_ch) and Wd.shape == (z_ch, dis_dim) and b.shape == (z_ch,)
    assert T.dtype == Wd.dtype == b.dtype == torch.float32
    idx = torch.randint(0, n_e, (rows,))
    s = torch.randn(rows, dis_dim)
    with torch.no_grad():
        ref = conv(torch.cat([E[idx], s], 1)[:, :, None, None])[:, :, 0, 0]
    got = T[idx] + s @ Wd.t() + b
    assert (got - ref).abs().max().item() <= 1e-6
