"""Cost of the Canny conditioning processor on the GPU.

    timeout -k 10 300 python tools/controlnet_bench.py --part kernel
    timeout -k 10 900 python tools/controlnet_bench.py --part engine

Random-init weights and synthetic frames; nothing is read from disk.

kernel  ops.canny_hint at --size (512x512) for B = 1 and B = 8 and reach
        0 / 16 / 32, writing f16 into a preallocated output from
        device-resident frames (blobs, a faint stripe and noise, so the
        hysteresis has chains to follow). Device events around --iters
        back-to-back calls, --reps windows per variant, the variants
        alternating inside each repetition; the median window per call with
        its min and max. One JSON line per (B, reach).

engine  ms/frame of the sd15 4-step 512x512 engine with use_controlnet,
        controlnet_processor "none" against "canny", both with pipelined
        graphs. Each window is --frames calls ended by a device
        synchronise, the two engines alternating, --reps windows each after
        a warm-up that includes the capture. One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ai_rtc_agent_amd import ops  # noqa: E402
from ai_rtc_agent_amd.config import EngineConfig  # noqa: E402
from ai_rtc_agent_amd.engine import StreamDiffusionEngine  # noqa: E402


def synthetic_frames(n, h, w, seed=0):
    """(n,h,w,3) u8: bold and faint discs, one faint stripe, sigma 3 noise."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32),
                            torch.arange(w, dtype=torch.float32), indexing="ij")
    out = []
    for _ in range(n):
        img = torch.full((h, w), 90.0)
        for c in (110.0, 24.0, 90.0, 20.0, 28.0, 60.0):
            cy, cx, r = torch.rand(3, generator=g).tolist()
            r = (0.05 + 0.2 * r) * min(h, w)
            img = torch.where((yy - cy * h) ** 2 + (xx - cx * w) ** 2 < r * r, img + c, img)
        img = torch.where(yy >= h // 2, img + 26.0, img)
        img = img + 3.0 * torch.randn((h, w), generator=g)
        out.append(img.round().clamp(0, 255).to(torch.uint8))
    return torch.stack(out).unsqueeze(-1).repeat(1, 1, 1, 3).contiguous()


def window_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def part_kernel(args):
    h, w = map(int, args.size.split("x"))
    for B in (1, 8):
        x = synthetic_frames(B, h, w).cuda()
        thr = torch.tensor([[args.low, args.high]] * B, dtype=torch.int32, device="cuda")
        out = torch.empty(x.shape, dtype=torch.float16, device="cuda")
        variants = {
            r: (lambda r=r: ops.canny_hint(x, thr, r, torch.float16, out=out))
            for r in (0, 16, 32)}
        frac = {}
        for r, fn in variants.items():  # warm-up: code objects
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            frac[r] = round(float(out[..., 0].float().mean()), 4)
        t = {r: [] for r in variants}
        for _ in range(args.reps):
            for r, fn in variants.items():
                t[r].append(window_us(fn, args.iters))
        for r, v in t.items():
            print(json.dumps({
                "metric": "canny_hint_us", "size": [h, w], "batch": B, "reach": r,
                "thresholds": [args.low, args.high], "edge_fraction": frac[r],
                "us": round(statistics.median(v), 2),
                "us_min_max": [round(min(v), 2), round(max(v), 2)],
                "iters": args.iters, "reps": args.reps,
                "device": torch.cuda.get_device_name(0)}), flush=True)


def part_engine(args):
    frames = synthetic_frames(8, 512, 512, seed=1).cuda()
    engines = {}
    for proc in ("none", "canny"):
        cfg = EngineConfig(model_family="sd15", width=512, height=512, device="cuda",
                           use_controlnet=True, controlnet_processor=proc,
                           canny_low=args.low, canny_high=args.high)
        eng = StreamDiffusionEngine(cfg)
        eng.prepare()
        for i in range(args.warmup):  # includes the capture
            eng(frames[i % len(frames)])
        eng.sync_output()
        torch.cuda.synchronize()
        engines[proc] = eng

    def window_ms(eng):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.frames):
            eng(frames[i % len(frames)])
        eng.sync_output()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.frames

    t = {k: [] for k in engines}
    for _ in range(args.reps):
        for k, eng in engines.items():
            t[k].append(window_ms(eng))
    rec = {"metric": "controlnet_engine_ms_per_frame", "family": "sd15",
           "size": [512, 512], "steps": 4, "frames": args.frames,
           "reps": args.reps, "canny_reach": engines["canny"].cfg.canny_reach}
    for k, v in t.items():
        rec[k + "_ms"] = round(statistics.median(v), 3)
        rec[k + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
    rec["canny_over_none"] = round(rec["canny_ms"] / rec["none_ms"], 4)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "engine"], required=True)
    ap.add_argument("--size", default="512x512", help="HxW for --part kernel")
    ap.add_argument("--low", type=int, default=100)
    ap.add_argument("--high", type=int, default=200)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops.hip_ext() is None:
        raise SystemExit("controlnet_bench needs a GPU and the built HIP extension")
    (part_kernel if args.part == "kernel" else part_engine)(args)


if __name__ == "__main__":
    main()
