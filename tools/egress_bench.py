"""Cost of the any-resolution egress (ops.unfit_frame_u8) on the GPU.

    python tools/egress_bench.py [--engine 512x512] [--iters 500] [--reps 9]

For each case (a 512x512 engine frame back to 1280x720 `contain`, and back
to 720x720 `cover`) three ways of producing the outgoing frame are timed:

  (a) rgb        RGB egress: one fit_resize_u8 launch
  (b) i420_fused the fused kernel: one fit_resize_u8_i420 launch
  (c) i420_two   what (b) replaces: RGB egress, then rgb_u8_to_i420

All write into preallocated outputs from the same device-resident frame.
Timing: device events around `--iters` back-to-back calls, `--reps` windows
per variant, the variants alternating inside each repetition; the median
window is reported per call with its min and max. (b) and (c) are checked
to give the same bytes. Prints one JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ai_rtc_agent_amd import ops  # noqa: E402

CASES = [((720, 1280), "contain"), ((720, 1280), "cover")]


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
    ap.add_argument("--engine", default="512x512", help="HxW of the engine frame")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available() or ops.hip_ext() is None:
        raise SystemExit("egress_bench needs a GPU and the built HIP extension")
    h, w = map(int, args.engine.split("x"))
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda()

    for (hs, ws), mode in CASES:
        window, (ht, wt) = ops.unfit_geometry(hs, ws, h, w, mode, even=True)
        rgb = torch.empty((ht, wt, 3), dtype=torch.uint8, device="cuda")
        rgb2 = torch.empty_like(rgb)
        yuv_f = torch.empty((ht // 2 * 3, wt), dtype=torch.uint8, device="cuda")
        yuv_t = torch.empty_like(yuv_f)

        def a_rgb():
            ops.unfit_frame_u8(img, window, (ht, wt), "rgb", out=rgb)

        def b_fused():
            ops.unfit_frame_u8(img, window, (ht, wt), "i420", out=yuv_f)

        def c_two():
            ops.unfit_frame_u8(img, window, (ht, wt), "rgb", out=rgb2)
            ops.rgb_u8_to_i420(rgb2, out=yuv_t)

        variants = {"rgb": a_rgb, "i420_fused": b_fused, "i420_two": c_two}
        for fn in variants.values():  # warm-up: code objects
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(yuv_f, yuv_t))
        t = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, fn in variants.items():
                t[k].append(window_us(fn, args.iters))
        rec = {"metric": "unfit_frame_u8_us", "engine": [h, w],
               "source": [hs, ws], "mode": mode, "window": list(window),
               "target": [ht, wt], "iters": args.iters, "reps": args.reps}
        for k, v in t.items():
            rec[k + "_us"] = round(statistics.median(v), 2)
            rec[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        rec["fused_over_two"] = round(rec["i420_fused_us"] / rec["i420_two_us"], 3)
        rec["fused_equals_two"] = same
        rec["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(rec), flush=True)
        if not same:
            raise SystemExit("fused I420 differs from the two-launch composition")


if __name__ == "__main__":
    main()
