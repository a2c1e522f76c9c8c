"""Checkpoint loading: diffusers-format weights -> our NHWC-functional models.

A user of the reference points `--model-id` at a diffusers repo
(lykon/dreamshaper-8) and weights load through the diffusers stack
(reference lib/wrapper.py:645-707). We load the same artifacts directly:
safetensors state dicts in diffusers' UNet2DConditionModel / TAESD naming,
remapped to this package's module tree. No diffusers dependency.

Offline note: real checkpoints are unfetchable in the build environment;
the mapping is exercised by tests that synthesize a diffusers-shaped state
dict for the tiny config and assert numerically-identical forwards are
impossible to get wrong silently (strict key coverage).
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import torch

from .unet import UNet2DCondition, UNetConfig


def _resnet_map(prefix_src: str, prefix_dst: str) -> List[Tuple[str, str]]:
    return [
        (f"{prefix_src}.norm1.weight", f"{prefix_dst}.norm1.weight"),
        (f"{prefix_src}.norm1.bias", f"{prefix_dst}.norm1.bias"),
        (f"{prefix_src}.conv1.weight", f"{prefix_dst}.conv1.weight"),
        (f"{prefix_src}.conv1.bias", f"{prefix_dst}.conv1.bias"),
        (f"{prefix_src}.time_emb_proj.weight", f"{prefix_dst}.time_emb_proj.weight"),
        (f"{prefix_src}.time_emb_proj.bias", f"{prefix_dst}.time_emb_proj.bias"),
        (f"{prefix_src}.norm2.weight", f"{prefix_dst}.norm2.weight"),
        (f"{prefix_src}.norm2.bias", f"{prefix_dst}.norm2.bias"),
        (f"{prefix_src}.conv2.weight", f"{prefix_dst}.conv2.weight"),
        (f"{prefix_src}.conv2.bias", f"{prefix_dst}.conv2.bias"),
        (f"{prefix_src}.conv_shortcut.weight", f"{prefix_dst}.shortcut.weight"),
        (f"{prefix_src}.conv_shortcut.bias", f"{prefix_dst}.shortcut.bias"),
    ]


def _attnblock_map(src: str, dst: str) -> List[Tuple[str, str]]:
    """diffusers Transformer2DModel -> our SpatialTransformer."""
    pairs = [
        (f"{src}.norm.weight", f"{dst}.norm.weight"),
        (f"{src}.norm.bias", f"{dst}.norm.bias"),
        (f"{src}.proj_in.weight", f"{dst}.proj_in.weight"),
        (f"{src}.proj_in.bias", f"{dst}.proj_in.bias"),
        (f"{src}.proj_out.weight", f"{dst}.proj_out.weight"),
        (f"{src}.proj_out.bias", f"{dst}.proj_out.bias"),
    ]
    return pairs


def _basic_block_map(src: str, dst: str) -> List[Tuple[str, str]]:
    pairs = []
    for a, b in (("attn1", "attn1"), ("attn2", "attn2")):
        pairs += [
            (f"{src}.{a}.to_q.weight", f"{dst}.{b}.to_q.weight"),
            (f"{src}.{a}.to_k.weight", f"{dst}.{b}.to_k.weight"),
            (f"{src}.{a}.to_v.weight", f"{dst}.{b}.to_v.weight"),
            (f"{src}.{a}.to_out.0.weight", f"{dst}.{b}.to_out.weight"),
            (f"{src}.{a}.to_out.0.bias", f"{dst}.{b}.to_out.bias"),
        ]
    pairs += [
        (f"{src}.norm1.weight", f"{dst}.norm1.weight"),
        (f"{src}.norm1.bias", f"{dst}.norm1.bias"),
        (f"{src}.norm2.weight", f"{dst}.norm2.weight"),
        (f"{src}.norm2.bias", f"{dst}.norm2.bias"),
        (f"{src}.norm3.weight", f"{dst}.norm3.weight"),
        (f"{src}.norm3.bias", f"{dst}.norm3.bias"),
        (f"{src}.ff.net.0.proj.weight", f"{dst}.ff.proj.weight"),
        (f"{src}.ff.net.0.proj.bias", f"{dst}.ff.proj.bias"),
        (f"{src}.ff.net.2.weight", f"{dst}.ff.out.weight"),
        (f"{src}.ff.net.2.bias", f"{dst}.ff.out.bias"),
    ]
    return pairs


def diffusers_unet_key_map(cfg: UNetConfig) -> List[Tuple[str, str]]:
    """Full (diffusers key -> our key) table for a UNet2DConditionModel."""
    pairs: List[Tuple[str, str]] = [
        ("conv_in.weight", "conv_in.weight"),
        ("conv_in.bias", "conv_in.bias"),
        ("time_embedding.linear_1.weight", "time_embed.0.weight"),
        ("time_embedding.linear_1.bias", "time_embed.0.bias"),
        ("time_embedding.linear_2.weight", "time_embed.1.weight"),
        ("time_embedding.linear_2.bias", "time_embed.1.bias"),
        ("conv_norm_out.weight", "norm_out.weight"),
        ("conv_norm_out.bias", "norm_out.bias"),
        ("conv_out.weight", "conv_out.weight"),
        ("conv_out.bias", "conv_out.bias"),
    ]
    if cfg.addition_embed_dim:
        pairs += [
            ("add_embedding.linear_1.weight", "add_embed.0.weight"),
            ("add_embedding.linear_1.bias", "add_embed.0.bias"),
            ("add_embedding.linear_2.weight", "add_embed.1.weight"),
            ("add_embedding.linear_2.bias", "add_embed.1.bias"),
        ]

    nblocks = len(cfg.block_out_channels)
    ri = 0  # flat resnet index in our down list
    for bi in range(nblocks):
        depth = cfg.transformer_depth[bi]
        for li in range(cfg.layers_per_block):
            src_r = f"down_blocks.{bi}.resnets.{li}"
            pairs += _resnet_map(src_r, f"down_resnets.{ri}")
            if depth > 0:
                src_a = f"down_blocks.{bi}.attentions.{li}"
                dst_a = f"down_attns.{ri}"
                pairs += _attnblock_map(src_a, dst_a)
                for d in range(depth):
                    pairs += _basic_block_map(
                        f"{src_a}.transformer_blocks.{d}", f"{dst_a}.blocks.{d}"
                    )
            ri += 1
        if bi < nblocks - 1:
            pairs += [
                (f"down_blocks.{bi}.downsamplers.0.conv.weight", f"downsamplers.{bi}.conv.weight"),
                (f"down_blocks.{bi}.downsamplers.0.conv.bias", f"downsamplers.{bi}.conv.bias"),
            ]

    pairs += _resnet_map("mid_block.resnets.0", "mid_res1")
    pairs += _resnet_map("mid_block.resnets.1", "mid_res2")
    pairs += _attnblock_map("mid_block.attentions.0", "mid_attn")
    mid_depth = max(1, cfg.transformer_depth[-1])
    for d in range(mid_depth):
        pairs += _basic_block_map(
            f"mid_block.attentions.0.transformer_blocks.{d}", f"mid_attn.blocks.{d}"
        )

    ri = 0
    for ui, bi in enumerate(reversed(range(nblocks))):
        depth = cfg.transformer_depth[bi]
        for li in range(cfg.layers_per_block + 1):
            pairs += _resnet_map(f"up_blocks.{ui}.resnets.{li}", f"up_resnets.{ri}")
            if depth > 0:
                src_a = f"up_blocks.{ui}.attentions.{li}"
                dst_a = f"up_attns.{ri}"
                pairs += _attnblock_map(src_a, dst_a)
                for d in range(depth):
                    pairs += _basic_block_map(
                        f"{src_a}.transformer_blocks.{d}", f"{dst_a}.blocks.{d}"
                    )
            ri += 1
        if ui < nblocks - 1:
            pairs += [
                (f"up_blocks.{ui}.upsamplers.0.conv.weight", f"upsamplers.{ui}.conv.weight"),
                (f"up_blocks.{ui}.upsamplers.0.conv.bias", f"upsamplers.{ui}.conv.bias"),
            ]
    return pairs


def load_diffusers_unet(
    model: UNet2DCondition, sd: Dict[str, torch.Tensor], strict: bool = True
) -> int:
    """Load a diffusers UNet2DConditionModel state dict into our model.

    Handles the proj_in/proj_out conv(1x1)-vs-linear difference: diffusers
    stores (C, C, 1, 1) convs for non-linear-projection models; ours stores
    whichever the config says.
    """
    own = dict(model.state_dict())
    loaded = 0
    missing: List[str] = []
    for src, dst in diffusers_unet_key_map(model.cfg):
        if src not in sd:
            if "shortcut" in dst:  # optional (only when channels change)
                continue
            missing.append(src)
            continue
        v = sd[src]
        tgt = own.get(dst)
        if tgt is None:
            if "shortcut" in dst:
                continue
            missing.append(src)
            continue
        if v.shape != tgt.shape:
            if v.dim() == 4 and v.shape[2] == 1 and tgt.dim() == 2:
                v = v[:, :, 0, 0]  # 1x1 conv -> linear
            elif v.dim() == 2 and tgt.dim() == 4:
                v = v[:, :, None, None]
            else:
                raise ValueError(f"shape mismatch {src}: {v.shape} vs {tgt.shape}")
        own[dst].copy_(v.to(own[dst].dtype))
        loaded += 1
    if strict and missing:
        raise KeyError(f"missing {len(missing)} keys, e.g. {missing[:5]}")
    return loaded


# TAESD sequential layouts. madebyollin/taesd ships two namings for the SAME
# flat-Sequential architecture:
#   raw   ("taesd_encoder/decoder.safetensors"):  encoder.N... / decoder.N...
#   diffusers AutoencoderTiny ("diffusion_pytorch_model.safetensors" at the
#   snapshot TOP LEVEL): encoder.layers.N... / decoder.layers.N...
# Encoder indices coincide (no parameter-free modules before conv_out);
# decoder indices differ by 1 (raw has a Clamp at 0 and a ReLU at 2, diffusers
# folds both into forward()). Each entry: (seq index, our module, is_block).
TAESD_SEQ_ENCODER = [
    (0, "conv_in", False),
    (1, "stage1", True),
    (2, "down1", False), (3, "stage2.0", True), (4, "stage2.1", True), (5, "stage2.2", True),
    (6, "down2", False), (7, "stage3.0", True), (8, "stage3.1", True), (9, "stage3.2", True),
    (10, "down3", False), (11, "stage4.0", True), (12, "stage4.1", True), (13, "stage4.2", True),
    (14, "conv_out", False),
]
TAESD_SEQ_DECODER_RAW = [
    (1, "conv_in", False),
    (3, "stage1.0", True), (4, "stage1.1", True), (5, "stage1.2", True),
    (7, "up1", False),
    (8, "stage2.0", True), (9, "stage2.1", True), (10, "stage2.2", True),
    (12, "up2", False),
    (13, "stage3.0", True), (14, "stage3.1", True), (15, "stage3.2", True),
    (17, "up3", False),
    (18, "stage4", True),
    (19, "conv_out", False),
]
TAESD_SEQ_DECODER_DIFFUSERS = [(i - 1, dst, b) for i, dst, b in TAESD_SEQ_DECODER_RAW]


def _load_taesd_seq(model, sd: Dict[str, torch.Tensor], prefix: str, table) -> int:
    """Copy a flat-Sequential TAESD state dict into one of our TAESD halves.

    Blocks are madebyollin _Block / diffusers AutoencoderTinyBlock: a `conv`
    Sequential whose parameterized entries are conv.0/conv.2/conv.4 → our
    c1/c2/c3."""
    own = dict(model.state_dict())
    n = 0
    for src_i, dst, is_block in table:
        if is_block:
            for ci, our in (("0", "c1"), ("2", "c2"), ("4", "c3")):
                for p in ("weight", "bias"):
                    k = f"{prefix}{src_i}.conv.{ci}.{p}"
                    ours = f"{dst}.{our}.{p}"
                    if k in sd and ours in own:
                        own[ours].copy_(sd[k].to(own[ours].dtype))
                        n += 1
        else:
            for p in ("weight", "bias"):
                k = f"{prefix}{src_i}.{p}"
                ours = f"{dst}.{p}"
                if k in sd and ours in own:
                    own[ours].copy_(sd[k].to(own[ours].dtype))
                    n += 1
    return n


def load_taesd_encoder(model, sd: Dict[str, torch.Tensor], prefix: str = "encoder.") -> int:
    if any(k.startswith(prefix + "layers.") for k in sd):
        prefix = prefix + "layers."
    return _load_taesd_seq(model, sd, prefix, TAESD_SEQ_ENCODER)


def load_taesd_decoder(model, sd: Dict[str, torch.Tensor], prefix: str = "decoder.") -> int:
    if any(k.startswith(prefix + "layers.") for k in sd):
        return _load_taesd_seq(model, sd, prefix + "layers.", TAESD_SEQ_DECODER_DIFFUSERS)
    return _load_taesd_seq(model, sd, prefix, TAESD_SEQ_DECODER_RAW)


def load_taesd(vae, sd: Dict[str, torch.Tensor]) -> Tuple[int, int]:
    """Load both halves of a TinyVAE from a combined TAESD state dict
    (either naming scheme). Returns (n_encoder, n_decoder) tensors loaded."""
    return (
        load_taesd_encoder(vae.encoder, sd, prefix="encoder."),
        load_taesd_decoder(vae.decoder, sd, prefix="decoder."),
    )


def _is_autoencoder_kl(sd: Dict[str, torch.Tensor]) -> bool:
    return any(k.startswith("encoder.down_blocks.") for k in sd)


# ---------------------------------------------------------------------------
# CLIP text encoder (transformers CLIPTextModel naming, as shipped in a
# diffusers snapshot's text_encoder/ directory — reference loads the same
# artifact via CLIPTextModel.from_pretrained, lib/wrapper.py:468-473)
# ---------------------------------------------------------------------------
def clip_text_key_map(n_layers: int) -> List[Tuple[str, str]]:
    pairs: List[Tuple[str, str]] = [
        ("text_model.embeddings.token_embedding.weight", "token_emb.weight"),
        ("text_model.embeddings.position_embedding.weight", "pos_emb.weight"),
        ("text_model.final_layer_norm.weight", "final_ln.weight"),
        ("text_model.final_layer_norm.bias", "final_ln.bias"),
    ]
    for i in range(n_layers):
        src = f"text_model.encoder.layers.{i}"
        dst = f"blocks.{i}"
        for a, b in (
            ("layer_norm1", "ln1"), ("layer_norm2", "ln2"),
            ("self_attn.q_proj", "q_proj"), ("self_attn.k_proj", "k_proj"),
            ("self_attn.v_proj", "v_proj"), ("self_attn.out_proj", "out_proj"),
            ("mlp.fc1", "fc1"), ("mlp.fc2", "fc2"),
        ):
            for p in ("weight", "bias"):
                pairs.append((f"{src}.{a}.{p}", f"{dst}.{b}.{p}"))
    pairs.append(("text_projection.weight", "pooled_proj.weight"))
    return pairs


def load_clip_text_encoder(model, sd: Dict[str, torch.Tensor],
                           strict: bool = False) -> int:
    """Load a CLIPTextModel state dict into our TextEncoder. With strict,
    every expected key (except the optional text_projection) must match."""
    own = dict(model.state_dict())
    n = 0
    missing: List[str] = []
    for src, dst in clip_text_key_map(len(model.blocks)):
        optional = dst.startswith("pooled_proj")
        # transformers <= 4.x serializes CLIPTextModel with a "text_model."
        # prefix (what shipped diffusers snapshots contain); 5.x dropped it
        v = sd.get(src)
        if v is None:
            v = sd.get(src.removeprefix("text_model."))
        if v is None or dst not in own:
            if not optional:
                missing.append(src)
            continue
        if v.shape != own[dst].shape:
            raise ValueError(f"shape mismatch {src}: {v.shape} vs {own[dst].shape}")
        own[dst].copy_(v.to(own[dst].dtype))
        n += 1
    if strict and missing:
        raise KeyError(f"missing {len(missing)} CLIP keys, e.g. {missing[:5]}")
    return n


# ---------------------------------------------------------------------------
# CLIP safety checker (CompVis/stable-diffusion-safety-checker; the
# safety_checker/ folder of SD1.5 snapshots). ClipSafetyChecker carries the
# checkpoint's own parameter names, so the map is name -> shape.
# ---------------------------------------------------------------------------
SAFETY_CHECKER_REPO = "CompVis/stable-diffusion-safety-checker"


def safety_checker_key_map(cfg=None) -> Dict[str, Tuple[int, ...]]:
    """Every tensor of a StableDiffusionSafetyChecker checkpoint for `cfg`
    (default: the published ViT-L/14 one), name -> shape."""
    from .safety_clip import ClipSafetyConfig

    cfg = cfg or ClipSafetyConfig()
    h, vt = cfg.hidden, "vision_model.vision_model"
    keys: Dict[str, Tuple[int, ...]] = {
        f"{vt}.embeddings.class_embedding": (h,),
        f"{vt}.embeddings.patch_embedding.weight": (h, 3, cfg.patch, cfg.patch),
        f"{vt}.embeddings.position_embedding.weight": (cfg.tokens, h),
        "visual_projection.weight": (cfg.projection, h),
        "concept_embeds": (cfg.concepts, cfg.projection),
        "special_care_embeds": (cfg.special, cfg.projection),
        "concept_embeds_weights": (cfg.concepts,),
        "special_care_embeds_weights": (cfg.special,),
    }
    for norm in ("pre_layrnorm", "post_layernorm"):
        keys[f"{vt}.{norm}.weight"] = keys[f"{vt}.{norm}.bias"] = (h,)
    for i in range(cfg.layers):
        p = f"{vt}.encoder.layers.{i}"
        for norm in ("layer_norm1", "layer_norm2"):
            keys[f"{p}.{norm}.weight"] = keys[f"{p}.{norm}.bias"] = (h,)
        for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
            keys[f"{p}.self_attn.{proj}.weight"] = (h, h)
            keys[f"{p}.self_attn.{proj}.bias"] = (h,)
        keys[f"{p}.mlp.fc1.weight"], keys[f"{p}.mlp.fc1.bias"] = (cfg.mlp, h), (cfg.mlp,)
        keys[f"{p}.mlp.fc2.weight"], keys[f"{p}.mlp.fc2.bias"] = (h, cfg.mlp), (h,)
    return keys


def load_safety_checker(model, sd: Dict[str, torch.Tensor]) -> int:
    """Load a StableDiffusionSafetyChecker state dict into a
    ClipSafetyChecker, strictly in both directions: a missing key, an
    unexpected key or a shape mismatch raises ValueError naming the keys
    (only a position_ids buffer is ignored, as older transformers versions
    serialise one). Sets model.weights = "loaded"."""
    sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
    want = safety_checker_key_map(model.cfg)
    missing = sorted(set(want) - set(sd))
    extra = sorted(set(sd) - set(want))
    if missing or extra:
        raise ValueError(
            f"safety checker checkpoint does not match: missing {missing}, "
            f"unexpected {extra}")
    bad = [f"{k}: {tuple(sd[k].shape)} vs {want[k]}" for k in sorted(want)
           if tuple(sd[k].shape) != want[k]]
    if bad:
        raise ValueError(f"safety checker shape mismatch: {bad}")
    own = dict(model.state_dict())
    with torch.no_grad():
        for k in want:
            own[k].copy_(sd[k].to(own[k].dtype))
    from ..ops import drop_weight_caches

    drop_weight_caches(model)
    model.weights = "loaded"
    return len(want)


def find_safety_checker_file(model_dir=None):
    """<model_dir>/safety_checker/model.safetensors, else the HF-cache
    snapshot of CompVis/stable-diffusion-safety-checker, else None."""
    import glob

    cands = []
    if model_dir:
        cands.append(os.path.join(model_dir, "safety_checker", "model.safetensors"))
    hub = os.environ.get("HF_HUB_CACHE", os.path.expanduser("~/.cache/huggingface/hub"))
    cands += sorted(glob.glob(os.path.join(
        hub, "models--" + SAFETY_CHECKER_REPO.replace("/", "--"), "snapshots",
        "*", "model.safetensors")))
    return next((p for p in cands if os.path.exists(p)), None)


def load_safety_checker_if_present(checker, model_dir=None) -> bool:
    """Fill a ClipSafetyChecker from the first checkpoint
    find_safety_checker_file offers; False (random init stays) when there
    is none or it does not match."""
    import logging

    from safetensors.torch import load_file

    from .safety_clip import ClipSafetyChecker

    if not isinstance(checker, ClipSafetyChecker) or checker.weights == "loaded":
        return False
    p = find_safety_checker_file(model_dir)
    if p is None:
        return False
    try:
        load_safety_checker(checker, load_file(p))
    except ValueError as e:
        logging.getLogger(__name__).warning(
            "safety checker checkpoint %s skipped: %s", p, e)
        return False
    return True


# ---------------------------------------------------------------------------
# AutoencoderKL (the vae/ folder of SD1.5 / SD2.1 / SD-Turbo snapshots) into
# models/vae_kl.py. Explicit map: checkpoint layer -> module path; the
# attention's to_q / to_k / to_v are packed into the module's one to_qkv.
# Unvalidated against a published snapshot until a weights volume exists
# (ROADMAP item 7); the synthetic round trip pins names and shapes.
# ---------------------------------------------------------------------------
_KL_ATTN_LEGACY = {"query": "to_q", "key": "to_k", "value": "to_v",
                   "proj_attn": "to_out.0"}


def autoencoder_kl_key_map(cfg) -> Tuple[Dict[str, str], Dict[str, str]]:
    """(layers, attentions) of a diffusers AutoencoderKL for `cfg`:
    layers maps a checkpoint layer prefix (it owns `.weight` and `.bias`) to
    the AutoencoderKLVAE submodule path; attentions maps a checkpoint
    attention prefix (group_norm, to_q, to_k, to_v, to_out.0 under it) to the
    _Attention module path."""
    layers: Dict[str, str] = {"quant_conv": "quant_conv",
                              "post_quant_conv": "post_quant_conv"}
    attns: Dict[str, str] = {}
    nb = len(cfg.block_out_channels)
    ch = cfg.block_out_channels

    def resnet(ck: str, own: str, shortcut: bool):
        for name in ("norm1", "conv1", "norm2", "conv2"):
            layers[f"{ck}.{name}"] = f"{own}.{name}"
        if shortcut:
            layers[f"{ck}.conv_shortcut"] = f"{own}.conv_shortcut"

    for side, blocks, per, sampler, own_sampler, widths in (
            ("encoder", "down_blocks", cfg.layers_per_block, "downsamplers",
             "downsample", ch),
            ("decoder", "up_blocks", cfg.layers_per_block + 1, "upsamplers",
             "upsample", tuple(reversed(ch)))):
        for name in ("conv_in", "conv_norm_out", "conv_out"):
            layers[f"{side}.{name}"] = f"{side}.{name}"
        for i in range(nb):
            cin = widths[max(i - 1, 0)]
            for j in range(per):
                resnet(f"{side}.{blocks}.{i}.resnets.{j}",
                       f"{side}.{blocks}.{i}.resnets.{j}",
                       j == 0 and cin != widths[i])
            if i < nb - 1:
                layers[f"{side}.{blocks}.{i}.{sampler}.0.conv"] = \
                    f"{side}.{blocks}.{i}.{own_sampler}"
        for j in (0, 1):
            resnet(f"{side}.mid_block.resnets.{j}",
                   f"{side}.mid_block.resnets.{j}", False)
        attns[f"{side}.mid_block.attentions.0"] = f"{side}.mid_block.attention"
    return layers, attns


def load_autoencoder_kl(vae, sd: Dict[str, torch.Tensor]) -> int:
    """Load a diffusers AutoencoderKL state dict into an AutoencoderKLVAE,
    strictly in both directions: every checkpoint key is consumed and every
    parameter filled, else ValueError naming the keys. The legacy attention
    names (query, key, value, proj_attn) and their 1x1-conv-shaped (C,C,1,1)
    weights are accepted. Returns the number of checkpoint tensors read."""
    layers, attns = autoencoder_kl_key_map(vae.cfg)
    sd = dict(sd)
    for k in list(sd):  # legacy attention names -> current ones
        for ap in attns:
            if k.startswith(ap + "."):
                head, _, leaf = k[len(ap) + 1:].rpartition(".")
                if head in _KL_ATTN_LEGACY:
                    sd[f"{ap}.{_KL_ATTN_LEGACY[head]}.{leaf}"] = sd.pop(k)
    own = dict(vae.named_parameters())
    plan = []        # (parameter name, tensor)
    used, missing = set(), []

    def take(key: str):
        if key not in sd:
            missing.append(key)
            return None
        used.add(key)
        return sd[key]

    def flat2(t):    # (C, C, 1, 1) conv-shaped linear weight -> (C, C)
        return t.reshape(t.shape[0], t.shape[1]) if t is not None and t.dim() == 4 else t

    for ck, path in layers.items():
        for leaf in ("weight", "bias"):
            plan.append((f"{path}.{leaf}", take(f"{ck}.{leaf}")))
    for ck, path in attns.items():
        for leaf in ("weight", "bias"):
            plan.append((f"{path}.group_norm.{leaf}", take(f"{ck}.group_norm.{leaf}")))
            parts = [take(f"{ck}.{n}.{leaf}") for n in ("to_q", "to_k", "to_v")]
            if leaf == "weight":
                parts = [flat2(t) for t in parts]
            plan.append((f"{path}.to_qkv.{leaf}",
                         None if any(t is None for t in parts)
                         else torch.cat(parts, dim=0)))
            out = take(f"{ck}.to_out.0.{leaf}")
            plan.append((f"{path}.to_out.{leaf}", flat2(out) if leaf == "weight" else out))
    extra = sorted(set(sd) - used)
    unfilled = sorted(set(own) - {name for name, _ in plan})
    if missing or extra or unfilled:
        raise ValueError(
            f"AutoencoderKL checkpoint does not match: missing {sorted(missing)}, "
            f"unexpected {extra}, parameters left unfilled {unfilled}")
    bad = [f"{name}: {tuple(t.shape)} vs {tuple(own[name].shape)}"
           for name, t in plan if tuple(t.shape) != tuple(own[name].shape)]
    if bad:
        raise ValueError(f"AutoencoderKL shape mismatch: {bad}")
    with torch.no_grad():
        for name, t in plan:
            own[name].copy_(t.to(own[name].dtype))
    from ..ops import drop_weight_caches

    drop_weight_caches(vae)
    return len(used)


def load_model_dir(engine, model_dir: str) -> bool:
    """Load UNet (+ TAESD enc+dec) safetensors from a local diffusers-style
    directory; returns False when nothing was found (random init stays).

    TAESD probe order matches what download.py actually fetches for
    madebyollin/taesd: the diffusers AutoencoderTiny file sits at the
    snapshot TOP LEVEL; the raw split files are taesd_encoder/decoder;
    dreamshaper-8's vae/ subdir is a full AutoencoderKL that cannot populate
    a TinyVAE — it is detected and skipped with a warning, unless the engine
    was built with use_tiny_vae=False: its AutoencoderKLVAE is then filled
    from that file (load_autoencoder_kl, strict) and TAESD files are passed
    over."""
    import logging

    from safetensors.torch import load_file

    log = logging.getLogger(__name__)
    found = False
    for sub in ("unet/diffusion_pytorch_model.safetensors", "unet.safetensors"):
        p = os.path.join(model_dir, sub)
        if os.path.exists(p):
            n = load_diffusers_unet(engine.unet, load_file(p), strict=False)
            if n == 0:
                log.warning("UNet checkpoint %s matched 0 tensors", p)
            else:
                found = True
            break
    from .vae_kl import AutoencoderKLVAE

    kl_vae = isinstance(getattr(engine, "vae", None), AutoencoderKLVAE)
    n_enc = n_dec = 0
    for sub in (
        "taesd.safetensors",
        "diffusion_pytorch_model.safetensors",  # AutoencoderTiny, top level
        "vae/diffusion_pytorch_model.safetensors",
    ):
        p = os.path.join(model_dir, sub)
        if not os.path.exists(p):
            continue
        sd = load_file(p)
        if _is_autoencoder_kl(sd) and kl_vae:
            # use_tiny_vae=False: the checkpoint's own VAE is the one wanted
            n_enc = n_dec = load_autoencoder_kl(engine.vae, sd)
            found = True
            break
        if kl_vae:
            continue  # a TAESD file cannot fill an AutoencoderKL
        if _is_autoencoder_kl(sd):
            log.warning("%s is a full AutoencoderKL, not TAESD; skipping "
                        "(fetch madebyollin/taesd for the TinyVAE weights)", p)
            continue
        n_enc, n_dec = load_taesd(engine.vae, sd)
        if n_enc or n_dec:
            found = True
            break
    # raw split files (madebyollin/taesd also ships these)
    if n_enc == 0 and not kl_vae:
        p = os.path.join(model_dir, "taesd_encoder.safetensors")
        if os.path.exists(p):
            n_enc = load_taesd_encoder(engine.vae.encoder, load_file(p), prefix="")
            found = found or n_enc > 0
    if n_dec == 0 and not kl_vae:
        p = os.path.join(model_dir, "taesd_decoder.safetensors")
        if os.path.exists(p):
            n_dec = load_taesd_decoder(engine.vae.decoder, load_file(p), prefix="")
            found = found or n_dec > 0
    if found and n_enc == 0 and n_dec == 0:
        log.warning("model dir %s: UNet loaded but no %s weights matched — "
                    "VAE stays random-init", model_dir,
                    "AutoencoderKL" if kl_vae else "TAESD")
    # CLIP text encoder(s) + BPE tokenizer(s)
    # (reference lib/wrapper.py:468-473; sdxl adds text_encoder_2)
    te = getattr(engine, "text_encoder", None)
    if te is not None:
        targets = [(te, "text_encoder")]
        if hasattr(te, "enc1") and hasattr(te, "enc2"):  # sdxl dual
            targets = [(te.enc1, "text_encoder"), (te.enc2, "text_encoder_2")]
        for mod, sub in targets:
            for fname in ("model.safetensors", "pytorch_model.safetensors"):
                p = os.path.join(model_dir, sub, fname)
                if os.path.exists(p):
                    try:
                        n = load_clip_text_encoder(mod, load_file(p))
                        if n:
                            found = True
                        else:
                            log.warning("CLIP checkpoint %s matched 0 tensors", p)
                    except ValueError as e:
                        log.warning("CLIP checkpoint %s skipped: %s", p, e)
                    break
        if hasattr(te, "load_tokenizer_dir") and te.load_tokenizer_dir(model_dir):
            log.info("BPE tokenizer loaded from %s", model_dir)
    # CLIP safety checker (reference lib/wrapper.py:930-942)
    if load_safety_checker_if_present(getattr(engine, "safety_checker", None),
                                      model_dir):
        found = True
    return found
