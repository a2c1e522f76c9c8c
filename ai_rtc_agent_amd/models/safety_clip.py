"""CLIP safety checker: the reference's StableDiffusionSafetyChecker.

Parity: the reference wrapper's one output-side safeguard (reference
lib/wrapper.py:290-298, 930-942) is a CLIP ViT-L/14 image tower with a
visual projection whose image embedding is compared, by cosine, with 17
concept embeddings and 3 "special care" embeddings; a flagged frame is
replaced by a black one. This module is that architecture with the
published checkpoint's parameter names
(CompVis/stable-diffusion-safety-checker, also the safety_checker/ folder
of SD1.5 snapshots), so the checkpoint loads 1:1 (models/load.py:
load_safety_checker).

Forward contract:
  1. patch embedding (a stride-`patch` conv without bias, run as a GEMM over
     ops.clip_patches rows)
  2. class token in front, position embedding added
  3. pre_layrnorm (sic: the checkpoint's spelling)
  4. `layers` pre-LN transformer blocks (quick_gelu MLPs)
  5. post_layernorm on the class token
  6. visual_projection (no bias)
  7. cosine against the two embedding tables

The decision law, in order (adj is the reference checker's `adjustment`,
positive = stricter):
  special_j = cos_j - special_care_embeds_weights_j + adj
  care      = 0.01 if any(special_j > 0) else 0
  concept_i = cos_i - concept_embeds_weights_i + adj + care
  flagged   = any(concept_i > 0)

On the GPU (f16) the blocks run q/k/v as one fused projection feeding
ops.attention's qkv layout, steps 5-7 and the law are one launch
(ops.safety_head) and flagged frames are blanked in place on the device
(ops.blank_flagged_): no host sync anywhere. On the CPU (f32) the same ops
take their torch forms.

Offline there is no checkpoint: the module is then random-init
(`weights == "random"`) and its verdicts mean nothing; the numerics are
verified against transformers.CLIPVisionModel and float64.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


@dataclass
class ClipSafetyConfig:
    """Defaults are the published checker: CLIP ViT-L/14."""

    image: int = 224
    patch: int = 14
    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    mlp: int = 4096
    projection: int = 768
    concepts: int = 17
    special: int = 3
    eps: float = 1e-5

    @property
    def tokens(self) -> int:
        return (self.image // self.patch) ** 2 + 1


class _Embeddings(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.randn(cfg.hidden))
        self.patch_embedding = nn.Conv2d(3, cfg.hidden, cfg.patch, cfg.patch, bias=False)
        self.position_embedding = nn.Embedding(cfg.tokens, cfg.hidden)


class _SelfAttention(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.heads = cfg.heads
        self.q_proj = nn.Linear(cfg.hidden, cfg.hidden)
        self.k_proj = nn.Linear(cfg.hidden, cfg.hidden)
        self.v_proj = nn.Linear(cfg.hidden, cfg.hidden)
        self.out_proj = nn.Linear(cfg.hidden, cfg.hidden)

    def _qkv(self):
        """(3*hidden, hidden) weight and (3*hidden,) bias of the fused
        projection, cached on the module."""
        w = ops.weight_cache(
            self, "_airtc_wqkv",
            lambda: torch.cat([self.q_proj.weight, self.k_proj.weight,
                               self.v_proj.weight], dim=0).detach().contiguous())
        b = ops.weight_cache(
            self, "_airtc_bqkv",
            lambda: torch.cat([self.q_proj.bias, self.k_proj.bias,
                               self.v_proj.bias], dim=0).detach().contiguous())
        return w, b

    def forward(self, h: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        w, b = self._qkv()
        q, k, v = F.linear(h, w, b).chunk(3, dim=-1)
        a = ops.attention(q, k, v, self.heads)
        return ops.linear(a, self.out_proj.weight, self.out_proj.bias,
                          residual=residual)


class _Mlp(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.fc1 = nn.Linear(cfg.hidden, cfg.mlp)
        self.fc2 = nn.Linear(cfg.mlp, cfg.hidden)


class _Layer(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.self_attn = _SelfAttention(cfg)
        self.layer_norm1 = nn.LayerNorm(cfg.hidden, eps=cfg.eps)
        self.mlp = _Mlp(cfg)
        self.layer_norm2 = nn.LayerNorm(cfg.hidden, eps=cfg.eps)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        n1, n2 = self.layer_norm1, self.layer_norm2
        x = self.self_attn(ops.layer_norm(x, n1.weight, n1.bias, n1.eps), x)
        h = F.linear(ops.layer_norm(x, n2.weight, n2.bias, n2.eps),
                     self.mlp.fc1.weight, self.mlp.fc1.bias)
        return ops.linear(ops.quick_gelu(h), self.mlp.fc2.weight,
                          self.mlp.fc2.bias, residual=x)


class _Encoder(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.layers)])


class _VisionTransformer(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden, eps=cfg.eps)
        self.encoder = _Encoder(cfg)
        self.post_layernorm = nn.LayerNorm(cfg.hidden, eps=cfg.eps)


class _VisionModel(nn.Module):
    """The checkpoint nests CLIPVisionModel.vision_model inside the
    checker's own vision_model attribute."""

    def __init__(self, cfg: ClipSafetyConfig):
        super().__init__()
        self.vision_model = _VisionTransformer(cfg)


class ClipSafetyChecker(nn.Module):
    def __init__(self, cfg: ClipSafetyConfig | None = None, seed: int = 0):
        super().__init__()
        self.cfg = cfg = cfg or ClipSafetyConfig()
        if cfg.image % cfg.patch or cfg.hidden % cfg.heads:
            raise ValueError(
                "image must be a multiple of patch and hidden of heads")
        # "loaded" once load_safety_checker has filled every parameter
        self.weights = "random"
        # own generator state: building the checker never moves the global
        # one, so the rest of an engine initialises as it does without it
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            self.vision_model = _VisionModel(cfg)
            self.visual_projection = nn.Linear(cfg.hidden, cfg.projection, bias=False)
            emb = self.vision_model.vision_model.embeddings
            nn.init.normal_(emb.class_embedding, std=0.02)
            nn.init.normal_(emb.position_embedding.weight, std=0.02)
            self.concept_embeds = nn.Parameter(
                torch.randn(cfg.concepts, cfg.projection), requires_grad=False)
            self.special_care_embeds = nn.Parameter(
                torch.randn(cfg.special, cfg.projection), requires_grad=False)
            # random-init thresholds far above any cosine: flags nothing
            self.concept_embeds_weights = nn.Parameter(
                torch.full((cfg.concepts,), 2.0), requires_grad=False)
            self.special_care_embeds_weights = nn.Parameter(
                torch.full((cfg.special,), 2.0), requires_grad=False)

    # ------------------------------------------------------------------
    @staticmethod
    def patchify(pixel_values: torch.Tensor, patch: int) -> torch.Tensor:
        """(B,3,S,S) normalised pixels -> (B, (S/patch)^2, 3*patch^2) rows in
        ops.clip_patches' (c, py, px) order."""
        B, C, S, _ = pixel_values.shape
        g = S // patch
        x = pixel_values.reshape(B, C, g, patch, g, patch)
        return x.permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * patch * patch)

    def tower(self, patches: torch.Tensor) -> torch.Tensor:
        """Steps 1-4: patch rows (B, N, 3*patch^2) -> hidden states
        (B, N + 1, hidden)."""
        vt = self.vision_model.vision_model
        emb = vt.embeddings
        w = emb.patch_embedding.weight
        x = F.linear(patches.to(w.dtype), w.reshape(w.shape[0], -1))
        cls = emb.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + emb.position_embedding.weight
        n = vt.pre_layrnorm
        x = ops.layer_norm(x.contiguous(), n.weight, n.bias, n.eps)
        for layer in vt.encoder.layers:
            x = layer(x)
        return x

    def pooled(self, patches: torch.Tensor) -> torch.Tensor:
        """Step 5: CLIPVisionModel's pooler_output."""
        n = self.vision_model.vision_model.post_layernorm
        cls = self.tower(patches)[:, 0]
        return F.layer_norm(cls.float(), (cls.shape[-1],), n.weight.float(),
                            n.bias.float(), n.eps).to(cls.dtype)

    def image_embeds(self, patches: torch.Tensor) -> torch.Tensor:
        """Step 6."""
        return F.linear(self.pooled(patches), self.visual_projection.weight)

    @torch.no_grad()
    def check_patches(self, patches: torch.Tensor, adjust: torch.Tensor,
                      counters: torch.Tensor):
        """Patch rows -> (flags int32 (B,), scores f32 (B, special +
        concepts)); counters[b] += flags[b]."""
        n = self.vision_model.vision_model.post_layernorm
        return ops.safety_head(
            self.tower(patches)[:, 0], n.weight, n.bias,
            self.visual_projection.weight, self.concept_embeds,
            self.concept_embeds_weights, self.special_care_embeds,
            self.special_care_embeds_weights, adjust, counters, n.eps)

    @torch.no_grad()
    def check(self, img: torch.Tensor, adjust: torch.Tensor | None = None,
              counters: torch.Tensor | None = None):
        """img: (B,H,W,3) in [-1,1], any H, W >= 8 -> (flags, scores)."""
        B = img.shape[0]
        if adjust is None:
            adjust = torch.zeros(B, dtype=torch.float32, device=img.device)
        if counters is None:
            counters = torch.zeros(B, dtype=torch.int32, device=img.device)
        patches = ops.clip_patches(img, self.cfg.image, self.cfg.patch)
        return self.check_patches(patches, adjust, counters)

    @torch.no_grad()
    def filter_(self, img: torch.Tensor, adjust: torch.Tensor | None = None,
                counters: torch.Tensor | None = None) -> torch.Tensor:
        """Blank (black, -1) every flagged frame of img IN PLACE: the
        reference's black-image substitution, decided and applied on the
        device."""
        flags, _ = self.check(img, adjust, counters)
        return ops.blank_flagged_(img, flags)
