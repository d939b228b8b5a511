"""HIP executors of the frozen VQ first stage: the encoder and, opt-in,
the decode path (quantizer lookup + post_quant_conv + Decoder, `VQDecoderExecutor` below).

`VQModelInterface.encode` = `quant_conv(encoder(x))` (autoencoder.py:313-316) with the
taming Encoder of model.py:368-459: conv_in, per level `num_res_blocks` ResnetBlocks
(GroupNorm(32, eps 1e-6) + swish + conv3x3, twice, + nin_shortcut when channels change),
a stride-2 Downsample between levels (F.pad(0,1,0,1) + conv k3 s2), mid ResnetBlock /
AttnBlock (single head over all pixels) / ResnetBlock, norm_out + swish, conv_out.
The reference runs it in fp32 (1.25 GFLOP/img, 16 % of the step's FLOPs) through
cuDNN/MIOpen with ~100 launches.  Here it is a static schedule over NHWC bf16 buffers on
the same kernels as the UNet: implicit-im2col MFMA GEMMs (the stride-2 pad-right
Downsample is an im2col mode), GroupNorm+swish, the MFMA attention (dh = C), and the
N=3 output conv with quant_conv folded into its weights (both linear: W' = Wq W_out,
b' = Wq b_out + bq).  No gradient: the first stage is frozen (ddpm_enc.py:562-568).
Weights are packed to bf16 once and re-packed if any parameter is modified in place
(load_state_dict bumps the tensors' version counters).
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib as L
from . import ops
from .graph_loops import capture
from .ops import Geom
from .unet import GN_FROM_PRODUCER

BF16 = torch.bfloat16
VQ_GN_EPS = 1e-6  # Normalize (model.py:30-31)


class _VQExecutorBase:
    """What the encoder and decoder executors share: the packed-weight cache keyed on the
    parameters' version counters, the persistent per-batch-size buffer table, and the
    ResnetBlock / AttnBlock / GroupNorm(+swish) schedules of model.py."""

    def __init__(self, vq):
        self._gsts = {}
        self.vq = vq
        self.dev = next(vq.parameters()).device
        assert self.dev.type == "cuda", "the HIP VQ first stage needs the module on a HIP device"
        self._sig = None
        self._packed: Dict[str, torch.Tensor] = {}
        self._bufs: Dict[int, Dict[str, torch.Tensor]] = {}

    # ------------------------------------------------------------ weights
    def _signature(self):
        return tuple(p._version for p in self.vq.parameters())

    @staticmethod
    def _conv_cl(w: torch.Tensor) -> torch.Tensor:
        """[co][ci][3][3] fp32 -> [co][9*ci] bf16 (channels-last taps, the GEMM B layout)."""
        return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(BF16).contiguous()

    def _pack_resblock(self, P, key, blk):
        P[key + ".conv1"] = self._conv_cl(blk.conv1.weight)
        P[key + ".conv2"] = self._conv_cl(blk.conv2.weight)
        if hasattr(blk, "nin_shortcut"):
            P[key + ".nin"] = blk.nin_shortcut.weight.detach()[:, :, 0, 0].to(BF16).contiguous()

    @staticmethod
    def _pack_attn(P, a):
        P["attn.qkv"] = torch.cat([a.q.weight, a.k.weight, a.v.weight], 0).detach()[:, :, 0, 0].to(BF16).contiguous()
        P["attn.qkv_b"] = torch.cat([a.q.bias, a.k.bias, a.v.bias], 0).detach().float().contiguous()
        P["attn.proj"] = a.proj_out.weight.detach()[:, :, 0, 0].to(BF16).contiguous()

    # ------------------------------------------------------------ buffers
    def _t(self, B: int, name: str, pixels: int, c: int, dtype=BF16) -> torch.Tensor:
        """Persistent per-(batch size, op) buffer: every op of the schedule owns its output
        (memory is not the constraint: ~0.3 GB at B=128), so graph replays are exact."""
        bufs = self._bufs.setdefault(B, {})
        t = bufs.get(name)
        if t is None or t.shape != (pixels, c) or t.dtype != dtype:
            t = bufs[name] = torch.empty(pixels, c, device=self.dev, dtype=dtype)
        return t

    # ------------------------------------------------------------ forward
    def _gst(self, B, name, out, g: Geom):
        """Producer-side GroupNorm statistics buffer for `out` (a GroupNorm input of >= 64
        pixels per image): the producing GEMM fills it, the GroupNorm skips its reduction."""
        if not GN_FROM_PRODUCER or g.h * g.w < 64 or (g.h * g.w) % 64:
            return None
        st = self._t(B, name + ".gst", 2 * g.pixels // 64, out.shape[1], torch.float32)
        self._gsts[out.data_ptr()] = st
        return st

    def _gn_swish(self, B, x, g: Geom, norm, name):
        out = self._t(B, name, g.pixels, x.shape[1])
        stats = self._t(B, "gn_stats", B, 2 * 32, torch.float32)
        ops.groupnorm_fwd(x, g, norm.weight, norm.bias, out, stats, VQ_GN_EPS, True, groups=norm.num_groups,
                          in_stats=self._gsts.get(x.data_ptr()))
        return out

    def _resblock(self, B, x, g: Geom, blk, key):
        """model.py ResnetBlock (temb None, dropout 0): shortcut(x) + conv2(sw(GN(conv1(sw(GN(x))))))."""
        cin, cout = blk.in_channels, blk.out_channels
        a = self._gn_swish(B, x, g, blk.norm1, key + ".a1")
        h = self._t(B, key + ".h", g.pixels, cout)
        ops.conv3x3_fwd(a, g, cin, self._packed[key + ".conv1"], h, bias=blk.conv1.bias,
                        gn_stats=self._gst(B, key + ".h", h, g))
        a2 = self._gn_swish(B, h, g, blk.norm2, key + ".a2")
        sc = x
        if cin != cout:
            sc = self._t(B, key + ".sc", g.pixels, cout)
            ops.linear_fwd(x, self._packed[key + ".nin"], sc, bias=blk.nin_shortcut.bias)
        out = self._t(B, key + ".out", g.pixels, cout)
        ops.conv3x3_fwd(a2, g, cout, self._packed[key + ".conv2"], out, bias=blk.conv2.bias, resid=sc,
                        gn_stats=self._gst(B, key + ".out", out, g))
        return out

    def _attn(self, B, x, g: Geom, attn):
        """model.py AttnBlock: x + proj_out(softmax(q k^T / sqrt(C)) v), one head over h*w."""
        c = x.shape[1]
        hn = self._gn_swish_free(B, x, g, attn.norm)
        qkv = self._t(B, "attn.qkv", g.pixels, 3 * c)
        ops.linear_fwd(hn, self._packed["attn.qkv"], qkv, bias=self._packed["attn.qkv_b"])
        o = self._t(B, "attn.o", g.pixels, c)
        lse = self._t(B, "attn.lse", B, g.h * g.w, torch.float32)
        ops.attention_fwd(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], o, lse, B, 1, g.h * g.w, g.h * g.w, c)
        out = self._t(B, "attn.out", g.pixels, c)
        ops.linear_fwd(o, self._packed["attn.proj"], out, bias=attn.proj_out.bias, resid=x,
                       gn_stats=self._gst(B, "attn.out", out, g))
        return out

    def _gn_swish_free(self, B, x, g, norm):
        out = self._t(B, "attn.norm", g.pixels, x.shape[1])
        stats = self._t(B, "gn_stats", B, 2 * 32, torch.float32)
        ops.groupnorm_fwd(x, g, norm.weight, norm.bias, out, stats, VQ_GN_EPS, False, groups=norm.num_groups,
                          in_stats=self._gsts.get(x.data_ptr()))
        return out


class VQEncoderExecutor(_VQExecutorBase):
    def __init__(self, vq):
        super().__init__(vq)
        enc = vq.encoder
        self.enc = enc
        for lvl in enc.down:
            if len(lvl.attn) > 0:
                raise NotImplementedError("attention inside down levels (attn_resolutions) is not on this path")

    def _pack(self):
        enc, P = self.enc, {}
        for i, lvl in enumerate(enc.down):
            for j, blk in enumerate(lvl.block):
                self._pack_resblock(P, f"d{i}.{j}", blk)
            if hasattr(lvl, "downsample"):
                P[f"d{i}.down"] = self._conv_cl(lvl.downsample.conv.weight)
        for name in ("block_1", "block_2"):
            self._pack_resblock(P, f"mid.{name}", getattr(enc.mid, name))
        P["conv_in"] = ops.pack_conv_pad8(enc.conv_in.weight)  # GEMM over channel-padded image rows
        self._pack_attn(P, enc.mid.attn_1)
        # conv_out followed by quant_conv (1x1): one 3x3 conv with composed weights (fp32)
        wq = self.vq.quant_conv.weight.detach()[:, :, 0, 0].float()
        P["out.w"] = torch.einsum("ij,jckl->ickl", wq, enc.conv_out.weight.detach().float()).contiguous()
        P["out.b"] = (wq @ enc.conv_out.bias.detach().float() + self.vq.quant_conv.bias.detach().float()).contiguous()
        self._packed = P
        self._sig = self._signature()

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """x fp32 NCHW [B, 3, R, R] in [-1, 1] -> quant_conv(encoder(x)) fp32 NCHW [B, z, R/f, R/f]."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, "HIP device fp32 NCHW input required"
        if self._sig != self._signature():
            self._pack()
        enc = self.enc
        B, _, R, _ = x.shape
        g = Geom(B, R, R)
        self._gsts = {}  # tensor -> statistics its producer wrote in THIS pass
        h = self._t(B, "conv_in", g.pixels, enc.ch)
        x8 = self._t(B, "x8", g.pixels, 8)
        ops.nchw_to_rows(x.contiguous(), 8, x8)
        ops.conv3x3_fwd(x8, g, 8, self._packed["conv_in"], h, bias=enc.conv_in.bias,
                        gn_stats=self._gst(B, "conv_in", h, g))
        for i, lvl in enumerate(enc.down):
            for j, blk in enumerate(lvl.block):
                h = self._resblock(B, h, g, blk, f"d{i}.{j}")
            if hasattr(lvl, "downsample"):
                c = h.shape[1]
                go = Geom(B, g.h // 2, g.w // 2)
                d = self._t(B, f"d{i}.down", go.pixels, c)
                ops.conv3x3_fwd(h, go, c, self._packed[f"d{i}.down"], d, bias=lvl.downsample.conv.bias,
                                resample=L.RESAMPLE_STRIDE2, gn_stats=self._gst(B, f"d{i}.down", d, go))
                h, g = d, go
        h = self._resblock(B, h, g, enc.mid.block_1, "mid.block_1")
        h = self._attn(B, h, g, enc.mid.attn_1)
        h = self._resblock(B, h, g, enc.mid.block_2, "mid.block_2")
        a = self._gn_swish(B, h, g, enc.norm_out, "norm_out")
        zc = self._packed["out.w"].shape[0]
        z = torch.empty(B, zc, g.h, g.w, device=self.dev, dtype=torch.float32)
        ops.small_conv_out_fwd(a, g, self._packed["out.w"], self._packed["out.b"], z)
        return z


class VQDecoderExecutor(_VQExecutorBase):
    """`VQModelInterface.decode` (autoencoder.py:328-369) on the HIP path: the quantizer's nearest-code
    lookup, the concat with the disentangled representation and post_quant_conv in one kernel
    (vq.hip; the 1x1 conv composed into a per-code table), then the taming Decoder
    (model.py:462-570) as a static schedule over NHWC bf16 buffers on the kernels the encoder
    uses: conv_in over the channel-padded rows, mid ResnetBlock / AttnBlock / ResnetBlock, per
    level from the top `num_res_blocks + 1` ResnetBlocks and an Upsample (nearest x2 as an im2col
    mode of its conv3x3), norm_out + swish, conv_out to fp32 NCHW.

    The first decode at a (batch shape, quantize?, representation?) runs eager; from the second
    on it replays a graph captured over the executor's static buffers (the input is copied in,
    the image cloned out).  A weight re-pack drops the graphs."""

    def __init__(self, vq):
        super().__init__(vq)
        dec = vq.decoder
        self.dec = dec
        for lvl in dec.up:
            if len(lvl.attn) > 0:
                raise NotImplementedError("attention inside up levels (attn_resolutions) is not on this path")
            if hasattr(lvl, "upsample") and not lvl.upsample.with_conv:
                raise NotImplementedError("Upsample without its conv (resamp_with_conv=False) is not on this path")
        if dec.give_pre_end or dec.tanh_out:
            raise NotImplementedError("give_pre_end / tanh_out are not on this path")
        self.e_dim = vq.quantize.e_dim
        self.dis_dim = vq.disentangled_dim if vq.use_disentangled_concat else 0
        if self.e_dim > ops.VQ_MAX_DIM or dec.conv_in.in_channels > 8:
            raise NotImplementedError("latents of more than 8 channels are not on this path")
        # a codebook beyond the lookup kernel's range keeps torch for the quantize step only
        self._lookup_hip = ops.vq_supported(vq.quantize.n_e, self.e_dim)
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self._calls: Dict[tuple, int] = {}
        self._hw: Dict[int, tuple] = {}

    # ------------------------------------------------------------ weights
    @staticmethod
    def pack_post_quant(codebook: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, e_dim: int):
        """post_quant_conv over cat(E[idx], s) is linear in both parts: returns (T, Wd, b) with
        T = E Wpq[:, :e_dim]^T [n_e][z_ch], Wd = Wpq[:, e_dim:] [z_ch][dis_dim] and the bias, fp32,
        so that the conv's output at a pixel is T[idx] + Wd s + b.  Device independent."""
        w = weight.detach()[:, :, 0, 0].float()
        T = codebook.detach().float() @ w[:, :e_dim].t()
        return T.contiguous(), w[:, e_dim:].contiguous(), bias.detach().float().contiguous()

    def _pack(self):
        dec, vq, P = self.dec, self.vq, {}
        P["conv_in"] = ops.pack_conv_pad8(dec.conv_in.weight)  # GEMM over the channel-padded latent rows
        for name in ("block_1", "block_2"):
            self._pack_resblock(P, f"mid.{name}", getattr(dec.mid, name))
        self._pack_attn(P, dec.mid.attn_1)
        for i, lvl in enumerate(dec.up):
            for j, blk in enumerate(lvl.block):
                self._pack_resblock(P, f"u{i}.{j}", blk)
            if hasattr(lvl, "upsample"):
                P[f"u{i}.up"] = self._conv_cl(lvl.upsample.conv.weight)
        P["out.w"] = dec.conv_out.weight.detach().float().contiguous()
        P["out.b"] = dec.conv_out.bias.detach().float().contiguous()
        E = vq.quantize.embedding.weight
        P["vq.codebook"] = E.detach().float().contiguous()
        P["vq.T"], P["vq.wd"], P["vq.b"] = self.pack_post_quant(E, vq.post_quant_conv.weight,
                                                                vq.post_quant_conv.bias, self.e_dim)
        P["vq.wq"] = vq.post_quant_conv.weight.detach()[:, :self.e_dim, 0, 0].float().contiguous()
        self._packed = P
        self._sig = self._signature()

    # ------------------------------------------------------------ forward
    def _static(self, B, H, W):
        dec = self.dec
        R = H * 2 ** (dec.num_resolutions - 1)
        oc = dec.conv_out.out_channels
        z = self._t(B, "z_in", B * self.e_dim, H * W, torch.float32).view(B, self.e_dim, H, W)
        s = self._t(B, "repr_in", B, max(self.dis_dim, 1), torch.float32)
        img = self._t(B, "img", B * oc, R * R, torch.float32).view(B, oc, R, R)
        return z, s, img

    def _run(self, B, H, W, quantize, has_repr):
        dec, P = self.dec, self._packed
        z, s, img = self._static(B, H, W)
        g = Geom(B, H, W)
        self._gsts = {}  # tensor -> statistics its producer wrote in THIS pass
        z8 = self._t(B, "z8", g.pixels, 8)
        head = dict(rows=z8, wd=P["vq.wd"], bias=P["vq.b"], repr=s if has_repr else None)
        if quantize and self._lookup_hip:
            ops.vq_lookup(z, P["vq.codebook"], table=P["vq.T"], **head)
        else:
            if quantize:
                z = self.vq.quantize(z)[0].contiguous()
            ops.vq_lookup(z, quantize=False, wq=P["vq.wq"], **head)
        h = self._t(B, "conv_in", g.pixels, dec.conv_in.out_channels)
        ops.conv3x3_fwd(z8, g, 8, P["conv_in"], h, bias=dec.conv_in.bias, gn_stats=self._gst(B, "conv_in", h, g))
        h = self._resblock(B, h, g, dec.mid.block_1, "mid.block_1")
        h = self._attn(B, h, g, dec.mid.attn_1)
        h = self._resblock(B, h, g, dec.mid.block_2, "mid.block_2")
        for i in reversed(range(dec.num_resolutions)):
            lvl = dec.up[i]
            for j, blk in enumerate(lvl.block):
                h = self._resblock(B, h, g, blk, f"u{i}.{j}")
            if hasattr(lvl, "upsample"):
                c = h.shape[1]
                go = Geom(B, 2 * g.h, 2 * g.w)
                u = self._t(B, f"u{i}.up", go.pixels, c)
                ops.conv3x3_fwd(h, go, c, P[f"u{i}.up"], u, bias=lvl.upsample.conv.bias,
                                resample=L.RESAMPLE_UP2, gn_stats=self._gst(B, f"u{i}.up", u, go))
                h, g = u, go
        a = self._gn_swish(B, h, g, dec.norm_out, "norm_out")
        ops.small_conv_out_fwd(a, g, P["out.w"], P["out.b"], img)
        return img

    @torch.no_grad()
    def decode(self, h: torch.Tensor, force_not_quantize=False, disentangled_repr=None) -> torch.Tensor:
        """h fp32 NCHW [B, e_dim, H, W] -> decoder(post_quant_conv(cat(quantize(h), repr))) fp32 NCHW."""
        assert h.is_cuda and h.dtype == torch.float32 and h.dim() == 4 and h.shape[1] == self.e_dim, \
            "HIP device fp32 NCHW latent required"
        if self._sig != self._signature():
            self._pack()
            self._graphs.clear()
            self._calls.clear()
        B, _, H, W = h.shape
        if self._hw.get(B) != (H, W):  # the buffers of this batch size change shape under its graphs
            for k in [k for k in self._graphs if k[0] == B]:
                del self._graphs[k]
            self._calls = {k: n for k, n in self._calls.items() if k[0] != B}
            self._hw[B] = (H, W)
        has_repr = disentangled_repr is not None and self.dis_dim > 0
        key = (B, H, W, not force_not_quantize, has_repr)
        z, s, img = self._static(B, H, W)
        z.copy_(h)
        if has_repr:
            assert disentangled_repr.shape == (B, self.dis_dim), "disentangled_repr [B, disentangled_dim] expected"
            s.copy_(disentangled_repr)
        n = self._calls.get(key, 0)
        self._calls[key] = n + 1
        if n == 0:
            self._run(*key)  # eager: also allocates buffers and library scratch outside a capture
        else:
            gr = self._graphs.get(key)
            if gr is None:
                ops.flush()
                gr = self._graphs[key] = capture(lambda: self._run(*key))  # warmed up by the first, eager call
            gr.replay()
        return img.clone()
