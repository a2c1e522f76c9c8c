"""What the CLIP safety checker costs per frame inside the decode graph.

    python tools/safety_bench.py [--fbs 1 8] [--frames 200] [--rounds 3]
                                 [--split] [--out FILE]

SD-Turbo 512x512, hipGraph on, pipelined, random weights. For every fbs two
engines are built on the same box, one without a checker and one with the
real-size ClipSafetyChecker (ViT-L/14, random weights), and timed in
alternating rounds of --frames calls each (host clock around work that ends
in a device synchronise). Reported per fbs: ms per call and per frame for
both, their difference, and the decode graph alone (stream B's replay of
_g2, timed with device events on an otherwise idle device), where the whole
checker lives.

--split adds a per-kernel table of one eager checker pass (torch.profiler
device times, averaged over 5 passes after 3 warm-up passes); it is taken
after the timings, tracing slows the host.

Needs a GPU: there is no CPU fallback, a timing from one would say nothing.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ai_rtc_agent_amd.config import sd_turbo_config  # noqa: E402
from ai_rtc_agent_amd.engine import StreamDiffusionEngine  # noqa: E402

# multiply-adds x 2 of the tower per frame, from the shapes
def tower_flops(cfg, tokens=None):
    n = tokens or cfg.tokens
    h, m = cfg.hidden, cfg.mlp
    per_layer = 2 * n * (4 * h * h + 2 * h * m) + 4 * n * n * h
    return cfg.layers * per_layer + 2 * (n - 1) * 3 * cfg.patch ** 2 * h


def make_engine(fbs, checker):
    cfg = sd_turbo_config(device="cuda", width=512, height=512,
                          frame_buffer_size=fbs, use_safety_checker=checker,
                          safety_checker="clip")
    eng = StreamDiffusionEngine(cfg)
    eng.prepare()
    return eng


def timed_calls(eng, frame, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        eng(frame)
    eng.sync_output()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def decode_graph_ms(eng, n):
    """The decode graph alone: replays of _g2[0] on stream B, device events."""
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(eng._sB):
        for _ in range(5):
            eng._g2[0].replay()
        start.record()
        for _ in range(n):
            eng._g2[0].replay()
        end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / n


def kernel_split(eng, fbs):
    from torch.profiler import ProfilerActivity, profile

    img = torch.rand(fbs, 512, 512, 3, device="cuda").half() * 2 - 1
    adj = torch.zeros(fbs, device="cuda")
    cnt = torch.zeros(fbs, dtype=torch.int32, device="cuda")
    for _ in range(3):
        eng.safety_checker.filter_(img, adj, cnt)
    torch.cuda.synchronize()
    passes = 5
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(passes):
            eng.safety_checker.filter_(img, adj, cnt)
        torch.cuda.synchronize()
    rows = []
    for ev in prof.key_averages():
        us = getattr(ev, "device_time_total", None)
        if us is None:
            us = getattr(ev, "cuda_time_total", 0.0)
        if us > 0:
            rows.append({"kernel": ev.key[:90], "launches_per_pass": ev.count / passes,
                         "us_per_pass": us / passes})
    rows.sort(key=lambda r: -r["us_per_pass"])
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--fbs", type=int, nargs="+", default=[1, 8])
    p.add_argument("--frames", type=int, default=200)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--split", action="store_true")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("safety_bench needs a GPU")

    result = {"device": torch.cuda.get_device_name(0), "frames": args.frames,
              "rounds": args.rounds, "cases": []}
    for fbs in args.fbs:
        g = torch.Generator().manual_seed(fbs)
        frame = torch.randint(0, 256, (fbs, 512, 512, 3), dtype=torch.uint8,
                              generator=g).cuda()
        off, on = make_engine(fbs, False), make_engine(fbs, True)
        for eng in (off, on):
            timed_calls(eng, frame, 30)  # capture + warm-up
        ms = {"off": [], "on": []}
        for _ in range(args.rounds):
            ms["off"].append(timed_calls(off, frame, args.frames))
            ms["on"].append(timed_calls(on, frame, args.frames))
        case = {
            "fbs": fbs,
            "call_ms_off": ms["off"], "call_ms_on": ms["on"],
            "frame_ms_off": min(ms["off"]) / fbs, "frame_ms_on": min(ms["on"]) / fbs,
            "decode_graph_ms_off": decode_graph_ms(off, 100),
            "decode_graph_ms_on": decode_graph_ms(on, 100),
            "tower_gflop_per_frame": tower_flops(on.safety_checker.cfg) / 1e9,
        }
        case["checker_ms_per_frame_in_decode_graph"] = (
            case["decode_graph_ms_on"] - case["decode_graph_ms_off"]) / fbs
        case["tower_tflops_in_decode_graph"] = (
            case["tower_gflop_per_frame"] / case["checker_ms_per_frame_in_decode_graph"])
        if args.split:
            try:
                case["kernels"] = kernel_split(on, fbs)
            except Exception as e:  # the profiler is optional equipment
                case["kernels"] = f"not measured: {type(e).__name__}: {e}"
        result["cases"].append(case)
        del off, on
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
