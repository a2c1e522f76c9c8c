#!/usr/bin/env python3
"""AOT engine build — parity with reference build.py:11-32.

The reference instantiates its wrapper with the production config
(dreamshaper-8 + LoRA at scale 1.0, LCM-LoRA, TinyVAE, img2img, fp16,
cfg "self") to force TensorRT engine compilation into the cache. Ours
builds the MI355X kernel plan: instantiate the engine (fusing LoRAs),
warm every kernel-side weight transform, capture the hipGraph once when a
GPU is present, and serialize the plan under ENGINES_CACHE/engines--<model>
(same directory contract as lib/wrapper.py:593-597).

    python build.py [--model-id ...] [--family sd15|sd21|sdxl] [--lora path:scale]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ai_rtc_agent_amd.config import EngineConfig, lora_adapter_specs
from ai_rtc_agent_amd.engine import StreamDiffusionEngine
from ai_rtc_agent_amd.engine.plan import save_plan


def build(
    model_id: str = "lykon/dreamshaper-8",
    family: str = "sd15",
    lora: dict | None = None,
    width: int = 512,
    full_vae: bool = False,
    lora_adapters: int | None = None,
    lora_max_rank: int | None = None,
    lora_adapter: list | None = None,
) -> str:
    cfg = EngineConfig(
        model_id=model_id,
        model_family=family,
        width=width,
        height=width,
        use_lcm_lora=True,
        use_tiny_vae=not full_vae,
        cfg_type="self",
        mode="img2img",
        lora_dict=lora,
        device="cuda" if torch.cuda.is_available() else "cpu",
        use_hip_graph=torch.cuda.is_available(),
    )
    # per-session LoRA bank: the plan gets its own cache key, and the named
    # adapter files are loaded once here so that a bad file fails the build,
    # not the server's start-up
    if lora_adapters is not None:
        cfg.lora_adapters = lora_adapters
    if lora_max_rank is not None:
        cfg.lora_max_rank = lora_max_rank
    cfg.__post_init__()
    specs = lora_adapter_specs(lora_adapter)
    if len(specs) > cfg.lora_adapters:
        raise ValueError(
            f"{len(specs)} LoRA adapters named, the bank holds "
            f"{cfg.lora_adapters} (--lora-adapters)")
    eng = StreamDiffusionEngine(cfg)
    eng.prepare()
    for i, (name, path, scale) in enumerate(specs):
        counts = eng.load_adapter(i, path, scale=scale, name=name)
        print(f"LoRA adapter {name!r} -> bank index {i}: {counts}")
    if torch.cuda.is_available():
        # warm the kernel-side weight transforms + capture the graph once
        frame = torch.zeros((width, width, 3), dtype=torch.uint8, device=cfg.device)
        eng(frame)
        torch.cuda.synchronize()
    out = save_plan(eng)
    print(f"engine plan written to {out}")
    return out


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--model-id", default="lykon/dreamshaper-8")
    p.add_argument("--family", default="sd15", choices=["sd15", "sd21", "sdxl", "tiny"])
    p.add_argument("--width", type=int, default=512)
    p.add_argument("--lora", default=None, help="path:scale[,path:scale...]")
    p.add_argument("--full-vae", action="store_true",
                   help="warm a plan with the checkpoint's full AutoencoderKL "
                        "(use_tiny_vae=False); it is cached beside the "
                        "tiny-VAE plan, under its own key")
    p.add_argument("--lora-adapters", type=int, default=None,
                   help="capacity of the per-session LoRA bank (0..64, "
                        "default $AIRTC_LORA_ADAPTERS or 0 = off)")
    p.add_argument("--lora-max-rank", type=int, default=None,
                   help="largest adapter rank the bank accepts (1..64)")
    p.add_argument("--lora-adapter", action="append", default=None,
                   metavar="NAME=PATH[:SCALE]",
                   help="check-load this adapter file into the bank; repeatable")
    a = p.parse_args()
    lora = None
    if a.lora:
        lora = {}
        for item in a.lora.split(","):
            path, _, scale = item.partition(":")
            lora[path] = float(scale or 1.0)
    build(a.model_id, a.family, lora, a.width, a.full_vae,
          a.lora_adapters, a.lora_max_rank, a.lora_adapter)
