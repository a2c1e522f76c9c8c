"""Shared helpers of test_vae_kl_cpu.py / test_vae_kl_gpu.py: an independent
functional float64 AutoencoderKL over a diffusers-named state dict, the seeded
generator of such state dicts, the d=512 attention case list and the bound
constants. Neither a conftest nor a test module; imports nothing from
models/vae_kl.py.

How the bounds are set (none is taken from the code under test):

attention d=512   |got - o| <= ATTN512_C * 2^-11 * (A + |o|), as for the
                  narrow kernels (_xfmr_ref). The wide kernel declares the
                  same arithmetic as attention.hip at a 64-key tile (f32
                  base-2 logits, online softmax from m = -1e30, P rounded to
                  f16 for PV only, f32 accumulation, f16 result), so
                  _xfmr_ref.attn_emulate(kt=64) is its emulator. Its maximum
                  ratio over ATTN512_CASES is ATTN512_EMU_MAX and ATTN512_C
                  is twice that (hardware exp2, MFMA order, the two partial
                  accumulators of S).
VAE f32 (CPU)     the module in f32 against the f64 reference: the f32-vs-f64
                  error of THIS reference run in f32 (VAE32_REF_ERR), times 4
                  for op-order differences.
VAE f16 (GPU)     VAE16_ERR is the error of this reference with every op's
                  output rounded to f16 once (`round16=True`, the declared
                  storage precision) against itself in f64; the GPU bound is
                  twice that, for relative RMS and for max-abs.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import _xfmr_ref as X

# ---------------------------------------------------------------------------
# configs
# ---------------------------------------------------------------------------


@dataclass(frozen=True)
class VaeCase:
    name: str
    block_out_channels: tuple
    layers_per_block: int
    norm_num_groups: int
    sizes: tuple            # (H, W) inputs the tests run
    latent_channels: int = 4
    scaling_factor: float = 0.18215

    @property
    def kwargs(self) -> dict:
        return dict(block_out_channels=self.block_out_channels,
                    layers_per_block=self.layers_per_block,
                    norm_num_groups=self.norm_num_groups,
                    latent_channels=self.latent_channels)

    @property
    def downscale(self) -> int:
        return 2 ** (len(self.block_out_channels) - 1)


# small: mid width 64 (the narrow attention kernel), one downsample.
# mid512: mid width 512 (the wide kernel); 32x32 gives 8x8 = 64 tokens, one
# exact kv tile; 40x24 gives 10x6 = 60, non-square and one ragged tile.
VAE_CASES = (
    VaeCase("small", (32, 64), 1, 8, ((16, 16),)),
    VaeCase("mid512", (32, 64, 512), 1, 8, ((32, 32), (40, 24))),
)


def vae_case(name: str) -> VaeCase:
    return next(c for c in VAE_CASES if c.name == name)


# measured by test_vae_kl_cpu.py (which fails if they go stale):
# (relative RMS, max abs) per (case, H, W, side)
VAE32_REF_ERR = {
    ("small", 16, 16, "encode"): (9.84e-07, 2.65e-07),
    ("small", 16, 16, "decode"): (6.47e-07, 1.62e-06),
    ("mid512", 32, 32, "encode"): (1.91e-06, 8.46e-07),
    ("mid512", 32, 32, "decode"): (1.46e-06, 4.58e-06),
    ("mid512", 40, 24, "encode"): (2.14e-06, 1.21e-06),
    ("mid512", 40, 24, "decode"): (1.47e-06, 4.57e-06),
}
VAE16_ERR = {
    ("small", 16, 16, "encode"): (9.95e-04, 2.78e-04),
    ("small", 16, 16, "decode"): (8.16e-04, 2.16e-03),
    ("mid512", 32, 32, "encode"): (9.97e-04, 5.60e-04),
    ("mid512", 32, 32, "decode"): (8.54e-04, 2.89e-03),
    ("mid512", 40, 24, "encode"): (1.01e-03, 6.03e-04),
    ("mid512", 40, 24, "decode"): (8.99e-04, 2.74e-03),
}
# how closely a recorded figure must match its re-measurement. f16 storage
# error moves only where a float64 sum lands on another side of a rounding
# boundary on another host; the f32 figures follow the host's summation
# order (thread count, vector width), hence a factor, not a percentage
VAE16_RTOL = 0.10
VAE32_FACTOR = 2.0


# ---------------------------------------------------------------------------
# seeded diffusers-named state dict
# ---------------------------------------------------------------------------

def kl_state_dict(case: VaeCase, seed: int = 0, legacy_attention: bool = False):
    """Every tensor of a diffusers AutoencoderKL for `case`, f32 values that
    f16 holds exactly (a model cast to f16 carries the same weights as the
    f64 reference). legacy_attention: the old names query/key/value/proj_attn
    with (C, C, 1, 1) weights."""
    g = torch.Generator().manual_seed(4100 + seed)
    sd = {}

    def f16exact(t):
        return t.half().float()

    def conv(p, cin, cout, k):
        sd[f"{p}.weight"] = f16exact(
            torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k))
        sd[f"{p}.bias"] = f16exact(torch.randn(cout, generator=g) * 0.1)

    def norm(p, c):
        sd[f"{p}.weight"] = f16exact(torch.randn(c, generator=g) * 0.2 + 1.0)
        sd[f"{p}.bias"] = f16exact(torch.randn(c, generator=g) * 0.1)

    def resnet(p, cin, cout):
        norm(f"{p}.norm1", cin)
        conv(f"{p}.conv1", cin, cout, 3)
        norm(f"{p}.norm2", cout)
        conv(f"{p}.conv2", cout, cout, 3)
        if cin != cout:
            conv(f"{p}.conv_shortcut", cin, cout, 1)

    def attn(p, c):
        norm(f"{p}.group_norm", c)
        names = (("query", "key", "value", "proj_attn") if legacy_attention
                 else ("to_q", "to_k", "to_v", "to_out.0"))
        for n in names:
            w = torch.randn(c, c, generator=g) / math.sqrt(c)
            sd[f"{p}.{n}.weight"] = f16exact(
                w[:, :, None, None] if legacy_attention else w)
            sd[f"{p}.{n}.bias"] = f16exact(torch.randn(c, generator=g) * 0.1)

    def mid(p, c):
        resnet(f"{p}.resnets.0", c, c)
        attn(f"{p}.attentions.0", c)
        resnet(f"{p}.resnets.1", c, c)

    ch, lc, n = case.block_out_channels, case.latent_channels, len(case.block_out_channels)
    conv("encoder.conv_in", 3, ch[0], 3)
    for i, c in enumerate(ch):
        cin = ch[max(i - 1, 0)]
        for j in range(case.layers_per_block):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}", cin if j == 0 else c, c)
        if i < n - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", c, c, 3)
    mid("encoder.mid_block", ch[-1])
    norm("encoder.conv_norm_out", ch[-1])
    conv("encoder.conv_out", ch[-1], 2 * lc, 3)
    conv("quant_conv", 2 * lc, 2 * lc, 1)
    conv("post_quant_conv", lc, lc, 1)
    rc = tuple(reversed(ch))
    conv("decoder.conv_in", lc, rc[0], 3)
    mid("decoder.mid_block", rc[0])
    for i, c in enumerate(rc):
        cin = rc[max(i - 1, 0)]
        for j in range(case.layers_per_block + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}", cin if j == 0 else c, c)
        if i < n - 1:
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c, c, 3)
    norm("decoder.conv_norm_out", rc[-1])
    conv("decoder.conv_out", rc[-1], 3, 3)
    return sd


# ---------------------------------------------------------------------------
# functional reference (NCHW inside, NHWC at the surface)
# ---------------------------------------------------------------------------

class _Ref:
    def __init__(self, sd, case: VaeCase, dtype, round16: bool):
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.case, self.dtype, self.round16 = case, dtype, round16

    def r(self, x):
        return x.half().to(self.dtype) if self.round16 else x

    def conv(self, x, p, stride=1, padding=1):
        return F.conv2d(x, self.sd[f"{p}.weight"], self.sd[f"{p}.bias"],
                        stride=stride, padding=padding)

    def norm(self, x, p, silu=True):
        y = F.group_norm(x, self.case.norm_num_groups, self.sd[f"{p}.weight"],
                         self.sd[f"{p}.bias"], eps=1e-6)
        return self.r(F.silu(y) if silu else y)

    def resnet(self, x, p):
        h = self.r(self.conv(self.norm(x, f"{p}.norm1"), f"{p}.conv1"))
        h = self.r(self.conv(self.norm(h, f"{p}.norm2"), f"{p}.conv2"))
        sc = x
        if f"{p}.conv_shortcut.weight" in self.sd:
            sc = self.r(self.conv(x, f"{p}.conv_shortcut", padding=0))
        return self.r(h + sc)

    def attn(self, x, p):
        b, c, h, w = x.shape
        t = self.norm(x, f"{p}.group_norm", silu=False)
        t = t.permute(0, 2, 3, 1).reshape(b, h * w, c)

        def lin(u, n):
            return self.r(u @ self.sd[f"{p}.{n}.weight"].t() + self.sd[f"{p}.{n}.bias"])

        q, k, v = lin(t, "to_q"), lin(t, "to_k"), lin(t, "to_v")
        pr = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(c), dim=-1)
        o = lin(self.r(pr @ v), "to_out.0")
        return self.r(o.reshape(b, h, w, c).permute(0, 3, 1, 2) + x)

    def mid(self, x, p):
        x = self.resnet(x, f"{p}.resnets.0")
        x = self.attn(x, f"{p}.attentions.0")
        return self.resnet(x, f"{p}.resnets.1")

    def encode(self, img):
        case, n = self.case, len(self.case.block_out_channels)
        x = self.r(self.conv(img.permute(0, 3, 1, 2).to(self.dtype), "encoder.conv_in"))
        for i in range(n):
            for j in range(case.layers_per_block):
                x = self.resnet(x, f"encoder.down_blocks.{i}.resnets.{j}")
            if i < n - 1:
                x = self.r(self.conv(F.pad(x, (0, 1, 0, 1)),
                                     f"encoder.down_blocks.{i}.downsamplers.0.conv",
                                     stride=2, padding=0))
        x = self.norm(self.mid(x, "encoder.mid_block"), "encoder.conv_norm_out")
        x = self.r(self.conv(x, "encoder.conv_out"))
        x = self.r(self.conv(x, "quant_conv", padding=0))
        mean = x[:, : case.latent_channels]
        return self.r(mean * case.scaling_factor).permute(0, 2, 3, 1).contiguous()

    def decode(self, z):
        case, n = self.case, len(self.case.block_out_channels)
        x = self.r(z.permute(0, 3, 1, 2).to(self.dtype) / case.scaling_factor)
        x = self.r(self.conv(x, "post_quant_conv", padding=0))
        x = self.r(self.conv(x, "decoder.conv_in"))
        x = self.mid(x, "decoder.mid_block")
        for i in range(n):
            for j in range(case.layers_per_block + 1):
                x = self.resnet(x, f"decoder.up_blocks.{i}.resnets.{j}")
            if i < n - 1:
                x = F.interpolate(x, scale_factor=2, mode="nearest")
                x = self.r(self.conv(x, f"decoder.up_blocks.{i}.upsamplers.0.conv"))
        x = self.norm(x, "decoder.conv_norm_out")
        return self.r(self.conv(x, "decoder.conv_out")).permute(0, 2, 3, 1).contiguous()


def kl_reference(sd, case: VaeCase, dtype=torch.float64, round16=False) -> _Ref:
    """The functional AutoencoderKL over `sd`: .encode(img NHWC) -> scaled
    mean latent NHWC, .decode(scaled latent NHWC) -> image NHWC. round16
    rounds every op's output to f16 once."""
    return _Ref(sd, case, dtype, round16)


def vae_inputs(case: VaeCase, H: int, W: int, batch: int = 2):
    """Seeded f16-exact (image in [-1, 1], scaled latent) NHWC, f32."""
    g = torch.Generator().manual_seed(4200 + 31 * H + W)
    img = (torch.rand(batch, H, W, 3, generator=g) * 2 - 1).half().float()
    s = case.downscale
    lat = (torch.randn(batch, H // s, W // s, case.latent_channels, generator=g)
           * case.scaling_factor * 4).half().float()
    return img, lat


@functools.lru_cache(maxsize=None)
def vae_reference(name: str, H: int, W: int):
    """(encode(img), decode(lat)) in float64, computed once and shared;
    callers do not write."""
    case = vae_case(name)
    ref = kl_reference(kl_state_dict(case), case)
    img, lat = vae_inputs(case, H, W)
    with torch.no_grad():
        return ref.encode(img), ref.decode(lat)


def vae_err(got: torch.Tensor, ref: torch.Tensor):
    """(relative RMS, max abs) of got against the float64 reference."""
    d = got.detach().cpu().double() - ref
    return (d.norm() / ref.norm()).item(), d.abs().max().item()


def vae_ref_err(name: str, H: int, W: int, dtype=torch.float64, round16=False):
    """The reference's own error when run in `dtype` / with f16 storage:
    {"encode": (rms, max), "decode": (rms, max)}."""
    case = vae_case(name)
    ref = kl_reference(kl_state_dict(case), case, dtype, round16)
    img, lat = vae_inputs(case, H, W)
    e64, d64 = vae_reference(name, H, W)
    with torch.no_grad():
        return {"encode": vae_err(ref.encode(img), e64),
                "decode": vae_err(ref.decode(lat), d64)}


# ---------------------------------------------------------------------------
# d = 512 attention
# ---------------------------------------------------------------------------

ATTN512_D = 512
ATTN512_KT = 64     # the wide kernel's kv tile

# measured by test_vae_kl_cpu.py (which fails if they go stale)
ATTN512_EMU_MAX = 0.806
ATTN512_C = 1.612


@dataclass(frozen=True)
class Attn512Case:
    name: str
    lq: int
    lk: int
    regime: str
    b: int = 2
    h: int = 1
    layout: str = "plain"   # plain | qkv

    @property
    def scale(self) -> float:
        return 1.0 / math.sqrt(ATTN512_D)


def _attn512_geometries():
    # ragged both ways with a second (16-row) q tile and more; one exact
    # tile; the smallest; a third tile of 2 keys; many tiles and a ragged 6
    g = [dict(name=f"lq{lq}-lk{lk}", lq=lq, lk=lk)
         for lq, lk in ((70, 77), (64, 64), (1, 1), (65, 130), (16, 1030))]
    # the VAE's layout: thirds of one packed projection, row stride 1536
    g.append(dict(name="qkv-l70", lq=70, lk=70, layout="qkv"))
    # two heads: the head stride
    g.append(dict(name="h2-lq70-lk77", lq=70, lk=77, b=1, h=2))
    return g


ATTN512_CASES = tuple(
    Attn512Case(**{**geo, "name": f"{geo['name']}-{r}"}, regime=r)
    for geo in _attn512_geometries() for r in X.REGIMES)


def attn512_case(name: str) -> Attn512Case:
    return next(c for c in ATTN512_CASES if c.name == name)


def attn512_inputs(case: Attn512Case, device="cpu"):
    """Seeded f16 (q, k, v) as (B, L, H*512) in the case's layout; the values
    are drawn on the CPU and do not depend on `device`."""
    g = torch.Generator().manual_seed(5120 + ATTN512_CASES.index(case))
    C = case.h * ATTN512_D
    qs = 6.0 if case.regime == "peaked" else 1.0
    vo = 3.0 if case.regime == "offset" else 0.0
    if case.layout == "qkv":
        t = torch.randn(case.b, case.lq, 3 * C, generator=g)
        t[..., :C] *= qs
        t[..., 2 * C:] += vo
        return t.half().to(device).chunk(3, dim=-1)
    q = (torch.randn(case.b, case.lq, C, generator=g) * qs).half().to(device)
    k = torch.randn(case.b, case.lk, C, generator=g).half().to(device)
    v = (torch.randn(case.b, case.lk, C, generator=g) + vo).half().to(device)
    return q, k, v


@functools.lru_cache(maxsize=None)
def attn512_reference(name: str):
    """(o, A) of a case in float64, computed once and shared."""
    case = attn512_case(name)
    q, k, v = attn512_inputs(case)
    return X.attn_ref64(q, k, v, case.h, case.scale)


def attn512_emulate(case: Attn512Case) -> torch.Tensor:
    q, k, v = attn512_inputs(case)
    return X.attn_emulate(q, k, v, case.h, case.scale, ATTN512_KT)
