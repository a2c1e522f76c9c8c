"""AOT kernel-plan cache — the TRT-engine-cache contract, MI355X-style.

The reference compiles TensorRT engines offline and caches them under
TRT_ENGINES_CACHE/engines--<model-id-with-dashes>/{unet,vae_encoder,
vae_decoder}.engine (reference lib/wrapper.py:585-597, 889-910;
Dockerfile:52). Our acceleration is hand-written HIP kernels + hipGraph
capture, so the cache holds what those need ahead of time:

engines--<model>/
    plan.json            engine config + kernel-plan metadata (shapes,
                         conv path/split-K decisions, attention dims)
    unet.safetensors     fused (LoRA-applied) UNet weights, fp16
    vae.safetensors      TinyVAE weights, fp16 (AutoencoderKL weights in
                         engines--<model>--full-vae/, use_tiny_vae=False)
    text_encoder.safetensors

Loading a plan skips model init + LoRA fusion; the hipGraph itself is
(re)captured in milliseconds at prepare() — capture is cheap once weights
and kernel decisions are fixed, which is what this cache pins down.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Optional

import torch

from ..config import EngineConfig, engines_cache_dir


def plan_dir(model_id: str, cache_root: Optional[str] = None,
             tiny_vae: bool = True, lora_adapters: int = 0) -> str:
    # naming contract: engines--<model-id with '/' -> '--'>; a plan built
    # with the checkpoint's full AutoencoderKL (use_tiny_vae=False) holds
    # other VAE weights under the same file name, so it gets its own key
    name = "engines--" + model_id.replace("/", "--")
    if not tiny_vae:
        name += "--full-vae"
    # an engine with a per-session adapter bank (lora_adapters > 0) runs other
    # graphs over the same weights: its own key as well
    if lora_adapters > 0:
        name += "--slot-lora"
    return os.path.join(cache_root or engines_cache_dir(), name)


def _cfg_dict(cfg: EngineConfig) -> dict:
    d = dataclasses.asdict(cfg)
    return d


def save_plan(engine, cache_root: Optional[str] = None) -> str:
    from safetensors.torch import save_file

    out = plan_dir(engine.cfg.model_id, cache_root, engine.cfg.use_tiny_vae,
                   engine.cfg.lora_adapters)
    os.makedirs(out, exist_ok=True)

    def dump(module: torch.nn.Module, name: str) -> None:
        sd = {k: v.detach().cpu().contiguous() for k, v in module.state_dict().items()}
        save_file(sd, os.path.join(out, name))

    dump(engine.unet, "unet.safetensors")
    dump(engine.vae, "vae.safetensors")
    dump(engine.text_encoder, "text_encoder.safetensors")

    meta = {
        "format": "airtc-plan-v1",
        "arch": "gfx950",
        "config": _cfg_dict(engine.cfg),
        "kernel_plan": kernel_plan_for(engine.cfg),
    }
    with open(os.path.join(out, "plan.json"), "w") as f:
        json.dump(meta, f, indent=2, default=str)
    return out


def load_plan(cfg: EngineConfig, cache_root: Optional[str] = None):
    """Build an engine from a cached plan; returns None when absent
    (callers fall back to fresh init — the reference's load-else-compile
    ladder, lib/wrapper.py:611-615)."""
    from safetensors.torch import load_file

    d = plan_dir(cfg.model_id, cache_root, cfg.use_tiny_vae, cfg.lora_adapters)
    if not os.path.exists(os.path.join(d, "plan.json")):
        return None
    from .engine import StreamDiffusionEngine

    with open(os.path.join(d, "plan.json")) as f:
        meta = json.load(f)
    saved = meta.get("config", {})
    cfg.model_family = saved.get("model_family", cfg.model_family)

    eng = StreamDiffusionEngine(
        dataclasses.replace(cfg, use_lcm_lora=False, lora_dict=None)
    )

    def restore(module: torch.nn.Module, name: str) -> None:
        sd = load_file(os.path.join(d, name))
        ref = dict(module.state_dict())
        module.load_state_dict(
            {k: v.to(dtype=ref[k].dtype) for k, v in sd.items()}, strict=True
        )

    restore(eng.unet.cpu(), "unet.safetensors")
    restore(eng.vae.cpu(), "vae.safetensors")
    restore(eng.text_encoder.cpu(), "text_encoder.safetensors")
    eng.unet = eng.unet.to(eng.device, eng.dtype)
    eng.vae = eng.vae.to(eng.device, eng.dtype)
    eng.text_encoder = eng.text_encoder.to(eng.device)
    return eng


def kernel_plan_for(cfg: EngineConfig) -> dict:
    """The AOT kernel decisions (what TRT would have baked into engines):
    conv geometry/split-K per layer class and attention head-dim handling.
    Recorded for inspection + warm-start; the runtime makes the same
    decisions deterministically (ops/csrc/conv2d.hip:airtc_conv2d_splitk_for)."""
    lat = cfg.latent_height
    plan = {
        "resolution": [cfg.height, cfg.width],
        "latent": [lat, cfg.latent_width],
        "unet_batch": cfg.unet_batch,
        "attention_head_dims": "32/64/96/128/160 native; others zero-padded",
        "vae": "taesd" if cfg.use_tiny_vae else
               "autoencoder_kl (mid-block attention: one 512-wide head)",
        "conv_paths": {
            "large_spatial": "BM128xBN64 MFMA, split-K to >=480 workgroups",
            "small_spatial": "BM64xBN64 MFMA, split-K to >=512 workgroups",
            "small_ic": "per-pixel OC-tile kernel (conv_in)",
        },
        "hip_graph": cfg.use_hip_graph,
    }
    if cfg.lora_adapters > 0:
        plan["slot_lora"] = {"adapters": cfg.lora_adapters,
                             "max_rank": cfg.lora_max_rank}
    return plan
