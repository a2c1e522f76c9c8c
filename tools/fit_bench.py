"""Cost of the fused any-resolution ingest kernel (ops.fit_frame_u8) against
the torch composite it replaces, on the GPU.

    python tools/fit_bench.py [--src 720x1280] [--dst 512x512] [--mode cover]

The composite is what an eager implementation has to launch: crop, permute,
float, antialiased interpolate, round, clamp, u8, permute, copy into the
slot. Both sides write the same slot of the same (B, H, W, 3) buffer from
the same device-resident source. Timing: device events around `--iters`
back-to-back calls, `--reps` windows per side, the two sides alternating;
the median window is reported per call. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ai_rtc_agent_amd import ops  # noqa: E402


def composite(src, out, slot, geom):
    (y0, x0, ch, cw), (oy, ox, oh, ow) = geom
    x = src[y0:y0 + ch, x0:x0 + cw].permute(2, 0, 1).unsqueeze(0).float()
    x = F.interpolate(x, size=(oh, ow), mode="bilinear", antialias=True,
                      align_corners=False)
    x = x.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
    if (oh, ow) != tuple(out.shape[1:3]):
        out[slot].zero_()
    out[slot, oy:oy + oh, ox:ox + ow].copy_(x)


def window_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default="720x1280", help="HxW of the source")
    ap.add_argument("--dst", default="512x512", help="HxW of the engine slot")
    ap.add_argument("--mode", default="cover", choices=ops.FIT_MODES)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops.hip_ext() is None:
        raise SystemExit("fit_bench needs a GPU and the built HIP extension")
    hs, ws = map(int, args.src.split("x"))
    h, w = map(int, args.dst.split("x"))
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (hs, ws, 3), generator=g, dtype=torch.uint8).cuda()
    out_k = torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda")
    out_t = torch.zeros_like(out_k)
    geom = ops.fit_geometry(hs, ws, h, w, args.mode)

    def fused():
        ops.fit_frame_u8(src, out_k, 1, args.mode)

    def torch_path():
        composite(src, out_t, 1, geom)

    for fn in (fused, torch_path):  # warm-up: code objects, allocator
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    d = (out_k.int() - out_t.int()).abs()
    t_f, t_t = [], []
    for _ in range(args.reps):
        t_f.append(window_us(fused, args.iters))
        t_t.append(window_us(torch_path, args.iters))
    fused_us, torch_us = statistics.median(t_f), statistics.median(t_t)
    print(json.dumps({
        "metric": "fit_frame_u8_us", "src": [hs, ws], "dst": [h, w],
        "mode": args.mode, "fused_us": round(fused_us, 2),
        "fused_us_min_max": [round(min(t_f), 2), round(max(t_f), 2)],
        "torch_composite_us": round(torch_us, 2),
        "torch_us_min_max": [round(min(t_t), 2), round(max(t_t), 2)],
        "speedup": round(torch_us / fused_us, 2),
        "max_abs_diff": int(d.max()),
        "frac_differing": round(float((d != 0).float().mean()), 5),
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
