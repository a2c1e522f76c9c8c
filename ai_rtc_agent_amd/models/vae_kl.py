"""AutoencoderKL — the VAE every SD1.5 / SD2.1 / SD-Turbo checkpoint ships,
from scratch, NHWC (`EngineConfig.use_tiny_vae=False`; the reference keeps
the pipeline's own AutoencoderKL then, lib/wrapper.py:699-707).

Same contract as TinyVAE (models/taesd.py): encode(img) returns the latent
times `scaling_factor`, decode(z) takes the same. The posterior MEAN is the
latent: deterministic and graph-friendly (the reference samples; the std of
a trained SD VAE is orders of magnitude below the mean's scale).

Every hot op goes through ai_rtc_agent_amd.ops: the NHWC MFMA conv (1x1
shortcut as a K-tail, nearest-2x in the A-load address, bottom/right-only
padding of the stride-2 downsamples as `pad_hi`), GroupNorm(+SiLU),
ops.linear, and for the mid-block's one head of width C the fused attention
kernels (C = 512: ops/csrc/attention_wide.hip), which read q, k, v as
strided views of one packed (3C, C) projection.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn as nn

from .. import ops

SD_LATENT_SCALE = 0.18215


@dataclass(frozen=True)
class KLConfig:
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    latent_channels: int = 4
    scaling_factor: float = SD_LATENT_SCALE
    image_channels: int = 3
    norm_eps: float = 1e-6

    def __post_init__(self):
        object.__setattr__(self, "block_out_channels",
                           tuple(int(c) for c in self.block_out_channels))
        if not self.block_out_channels or self.layers_per_block < 1:
            raise ValueError("AutoencoderKL needs at least one block and one "
                             "resnet per block")
        for c in self.block_out_channels:
            if c % self.norm_num_groups:
                raise ValueError(
                    f"block width {c} does not split into "
                    f"{self.norm_num_groups} GroupNorm groups")

    @property
    def mid_channels(self) -> int:
        return self.block_out_channels[-1]

    @property
    def downscale(self) -> int:
        return 2 ** (len(self.block_out_channels) - 1)


# the tiny model family's stand-in: four blocks (the engine's latent is 1/8
# of the frame), mid width 64
TINY_KL_CONFIG = KLConfig(block_out_channels=(32, 32, 64, 64),
                          layers_per_block=1, norm_num_groups=8)


class _Conv(nn.Module):
    """OIHW weight + bias over NHWC; pad_hi = extra bottom/right zero padding
    (ops.conv2d_nhwc)."""

    def __init__(self, cin: int, cout: int, k: int = 3, stride: int = 1,
                 padding: int | None = None, pad_hi: int = 0):
        super().__init__()
        self.stride, self.pad_hi = stride, pad_hi
        self.padding = k // 2 if padding is None else padding
        self.weight = nn.Parameter(
            torch.randn(cout, cin, k, k) / math.sqrt(cin * k * k))
        self.bias = nn.Parameter(torch.zeros(cout))

    def forward(self, x, residual=None, tail=None, upsample2x=False):
        return ops.conv2d_nhwc(x, self.weight, self.bias, self.stride,
                               self.padding, residual=residual, tail=tail,
                               upsample2x=upsample2x, pad_hi=self.pad_hi)


class _Norm(nn.Module):
    def __init__(self, c: int, cfg: KLConfig, silu: bool = True):
        super().__init__()
        self.groups, self.eps, self.silu = cfg.norm_num_groups, cfg.norm_eps, silu
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))

    def forward(self, x):
        return ops.group_norm_silu_nhwc(x, self.groups, self.weight, self.bias,
                                        self.eps, self.silu)


class _Resnet(nn.Module):
    """norm1-SiLU-conv1-norm2-SiLU-conv2 + input; no time embedding."""

    def __init__(self, cin: int, cout: int, cfg: KLConfig):
        super().__init__()
        self.norm1 = _Norm(cin, cfg)
        self.conv1 = _Conv(cin, cout)
        self.norm2 = _Norm(cout, cfg)
        self.conv2 = _Conv(cout, cout)
        self.conv_shortcut = _Conv(cin, cout, 1) if cin != cout else None

    def forward(self, x):
        h = self.conv1(self.norm1(x))
        h = self.norm2(h)
        if self.conv_shortcut is None:
            return self.conv2(h, residual=x)
        sc = self.conv_shortcut
        return self.conv2(h, tail=(x, sc.weight, sc.bias))


def _attention_unfused(q, k, v):
    """softmax(q k^T / sqrt(C)) v as bmm, f32 softmax, bmm: materialises the
    (B, L, L) logits."""
    s = torch.bmm(q, k.transpose(1, 2)).float() * (1.0 / math.sqrt(q.shape[-1]))
    return torch.bmm(torch.softmax(s, dim=-1).to(v.dtype), v)


class _Attention(nn.Module):
    """GroupNorm, one head of width C over the H*W tokens, out projection,
    residual. q, k, v come from ONE (3C, C) projection and reach the
    attention kernel as its strided thirds, zero-copy."""

    def __init__(self, c: int, cfg: KLConfig):
        super().__init__()
        self.group_norm = _Norm(c, cfg, silu=False)
        self.to_qkv = nn.Linear(c, 3 * c)
        self.to_out = nn.Linear(c, c)

    def forward(self, x):
        b, h, w, c = x.shape
        t = self.group_norm(x).reshape(b, h * w, c)
        qkv = ops.linear(t, self.to_qkv.weight, self.to_qkv.bias)
        q, k, v = qkv.chunk(3, dim=-1)
        route = os.environ.get("AIRTC_VAE_ATTN") or "hip"
        if route == "hip":
            o = ops.attention(q, k, v, 1)
        elif route == "unfused":
            # operator's switch, read per call: two library GEMMs around an
            # f32 softmax. On an MI355X this route measured about twice as
            # fast as the wide-head kernel (profiles/full_vae.md); the kernel
            # stays the default, as every hot path here is the project's own
            o = _attention_unfused(q, k, v)
        else:
            raise ValueError(
                f"AIRTC_VAE_ATTN must be 'hip' or 'unfused', got {route!r}")
        o = ops.linear(o, self.to_out.weight, self.to_out.bias,
                       residual=x.reshape(b, h * w, c))
        return o.reshape(b, h, w, c)


class _Mid(nn.Module):
    def __init__(self, c: int, cfg: KLConfig):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(c, c, cfg), _Resnet(c, c, cfg)])
        self.attention = _Attention(c, cfg)

    def forward(self, x):
        return self.resnets[1](self.attention(self.resnets[0](x)))


class _DownBlock(nn.Module):
    def __init__(self, cin: int, cout: int, cfg: KLConfig, down: bool):
        super().__init__()
        self.resnets = nn.ModuleList(
            [_Resnet(cin if j == 0 else cout, cout, cfg)
             for j in range(cfg.layers_per_block)])
        # diffusers: F.pad(x, (0, 1, 0, 1)) then 3x3 stride 2, padding 0
        self.downsample = (_Conv(cout, cout, 3, stride=2, padding=0, pad_hi=1)
                           if down else None)

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return x if self.downsample is None else self.downsample(x)


class _UpBlock(nn.Module):
    def __init__(self, cin: int, cout: int, cfg: KLConfig, up: bool):
        super().__init__()
        self.resnets = nn.ModuleList(
            [_Resnet(cin if j == 0 else cout, cout, cfg)
             for j in range(cfg.layers_per_block + 1)])
        self.upsample = _Conv(cout, cout, 3) if up else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return x if self.upsample is None else self.upsample(x, upsample2x=True)


class KLEncoder(nn.Module):
    """(B,H,W,3) -> (B,H/s,W/s,2*latent) moments, before quant_conv."""

    def __init__(self, cfg: KLConfig):
        super().__init__()
        ch = cfg.block_out_channels
        self.conv_in = _Conv(cfg.image_channels, ch[0])
        self.down_blocks = nn.ModuleList(
            [_DownBlock(ch[max(i - 1, 0)], c, cfg, down=i < len(ch) - 1)
             for i, c in enumerate(ch)])
        self.mid_block = _Mid(ch[-1], cfg)
        self.conv_norm_out = _Norm(ch[-1], cfg)
        self.conv_out = _Conv(ch[-1], 2 * cfg.latent_channels)

    def features(self, x):
        h = self.conv_in(x)
        for blk in self.down_blocks:
            h = blk(h)
        return self.conv_norm_out(self.mid_block(h))


class KLDecoder(nn.Module):
    """(B,h,w,latent), after post_quant_conv -> (B,s*h,s*w,3)."""

    def __init__(self, cfg: KLConfig):
        super().__init__()
        ch = tuple(reversed(cfg.block_out_channels))
        self.conv_in = _Conv(cfg.latent_channels, ch[0])
        self.mid_block = _Mid(ch[0], cfg)
        self.up_blocks = nn.ModuleList(
            [_UpBlock(ch[max(i - 1, 0)], c, cfg, up=i < len(ch) - 1)
             for i, c in enumerate(ch)])
        self.conv_norm_out = _Norm(ch[-1], cfg)
        self.conv_out = _Conv(ch[-1], cfg.image_channels)

    def forward(self, z):
        h = self.mid_block(self.conv_in(z))
        for blk in self.up_blocks:
            h = blk(h)
        return self.conv_out(self.conv_norm_out(h))


class AutoencoderKLVAE(nn.Module):
    """Paired encoder/decoder with the SD latent-scale contract.

    fold_encoder_tail: conv_out followed by quant_conv, restricted to the
    mean channels and times scaling_factor, is one linear map; it runs as ONE
    3x3 conv whose weight is composed at first use (ops.weight_cache, dropped
    with the other caches when weights change). False runs the three steps.
    post_quant_conv is NOT folded into the decoder's conv_in: its bias meets
    the 3x3's zero padding, so the composition is not exact at the border.
    """

    def __init__(self, cfg: KLConfig | None = None, *, fold_encoder_tail: bool = True,
                 device=None, **overrides):
        super().__init__()
        cfg = cfg if cfg is not None else KLConfig(**overrides)
        self.cfg = cfg
        self.scaling_factor = cfg.scaling_factor
        self.fold_encoder_tail = fold_encoder_tail
        self.encoder = KLEncoder(cfg)
        self.decoder = KLDecoder(cfg)
        lc = cfg.latent_channels
        self.quant_conv = _Conv(2 * lc, 2 * lc, 1)
        self.post_quant_conv = _Conv(lc, lc, 1)
        if device is not None and torch.device(device).type == "cuda":
            self.check_gpu_support()

    def check_gpu_support(self) -> None:
        """The mid block attends with one head of the last block's width: on
        the GPU that must be a width an attention kernel serves."""
        c = self.cfg.mid_channels
        if not ops.attention_serves(c):
            raise ValueError(
                f"AutoencoderKL mid-block width {c} is one attention head no "
                f"HIP kernel serves (up to 160, or 512)")

    def _folded_tail(self):
        co, qc = self.encoder.conv_out, self.quant_conv
        lc, sf = self.cfg.latent_channels, self.scaling_factor

        def build():
            wq = qc.weight.detach().float()[:lc, :, 0, 0]           # (lc, 2lc)
            w = torch.einsum("om,mirs->oirs", wq, co.weight.detach().float())
            b = wq @ co.bias.detach().float() + qc.bias.detach().float()[:lc]
            dt = co.weight.dtype
            return (w * sf).to(dt).contiguous(), (b * sf).to(dt).contiguous()

        return ops.weight_cache(
            self, "_airtc_kl_tail", build,
            key=(co.weight, co.bias, qc.weight, qc.bias, sf))

    def encode(self, img: torch.Tensor) -> torch.Tensor:
        if ops.uses_hip(img):
            self.check_gpu_support()
        h = self.encoder.features(img)
        if self.fold_encoder_tail:
            w, b = self._folded_tail()
            return ops.conv2d_nhwc(h, w, b, 1, 1)
        moments = self.quant_conv(self.encoder.conv_out(h))
        mean = moments[..., : self.cfg.latent_channels]
        return (mean * self.scaling_factor).contiguous()

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        if ops.uses_hip(z):
            self.check_gpu_support()
        z = (z / self.scaling_factor).contiguous()
        return self.decoder(self.post_quant_conv(z))
