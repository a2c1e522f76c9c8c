#!/usr/bin/env python3
"""RCFG-active benchmark: sd15 4-step, cfg self, guidance > 1.

`bench.py --model sd15` runs the production default guidance_scale = 0.0,
where the RCFG step is not in the captured graph at all. This tool times the
configuration in which it is (the row "RCFG active" of
profiles/optimization_ladder.md): EngineConfig defaults (sd15 geometry,
512x512, t_index_list [18, 26, 35, 45], cfg_type "self", LCM-LoRA fused,
hipGraph + pipeline overlap, no similarity filter) with guidance_scale set.
It also counts the kernel launches of one eager step, for this configuration
and for the headline SD-Turbo one (cfg none), whose count must not move.

usage: python tools/rcfg_bench.py [--guidance 1.5] [--steps 300] [--warmup 30]
prints one JSON line per configuration.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ai_rtc_agent_amd.config import EngineConfig, sd_turbo_config  # noqa: E402
from ai_rtc_agent_amd.engine import StreamDiffusionEngine  # noqa: E402


def count_launches(eng):
    """Kernel launches of one eager step (the work a captured graph holds)."""
    from torch.profiler import ProfilerActivity, profile

    eng._step_core()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        eng._step_core()
        torch.cuda.synchronize()
    return sum(
        1 for ev in prof.events()
        if ev.device_type == torch.autograd.DeviceType.CUDA
        and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())


def run(name, cfg, steps, warmup):
    eng = StreamDiffusionEngine(cfg)
    eng.prepare()
    g = torch.Generator().manual_seed(1234)
    frames = [torch.randint(0, 256, (cfg.height, cfg.width, 3), generator=g,
                            dtype=torch.uint8).cuda() for _ in range(4)]
    for i in range(warmup):
        eng(frames[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for i in range(steps):
        out = eng(frames[i % 4])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.sync_output()
    print(json.dumps({
        "config": name, "fps": round(steps / dt, 2),
        "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
        # same seed, same frames: equal checksums = equal last frame
        "checksum": int(out.to(torch.int64).sum().item()),
        "launches_per_eager_step": count_launches(eng)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--guidance", type=float, default=1.5)
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=30)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rcfg_bench needs a GPU: a CPU timing says nothing about it")
    run(f"sd15 4-step rcfg self g={args.guidance}",
        EngineConfig(device="cuda", guidance_scale=args.guidance),
        args.steps, args.warmup)
    run("sd-turbo 1-step cfg none", sd_turbo_config(device="cuda"),
        args.steps, args.warmup)


if __name__ == "__main__":
    main()
