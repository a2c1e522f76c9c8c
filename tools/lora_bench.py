#!/usr/bin/env python3
"""Cost of per-session LoRA on one GPU.

    python tools/lora_bench.py [--kernel] [--engine] [--frames N]

--kernel: ops.lora_delta_ against the obvious unfused route (gather by
row_adapter, two torch.bmm, add) at L = 4096, K = N = 320 and L = 256,
K = N = 1280, R = 32, 8 rows all assigned; both timed from CUDA graphs of 20
calls so that launch overhead on the host is not what is compared.
--engine: sd-turbo 512x512 at fbs = 8, capacity 4, R = 32: aggregate fps with
(a) lora_adapters = 0, (b) capacity on and no slot assigned (the early-exit
launches alone), (c) all eight slots assigned.
Prints one JSON line per figure.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ai_rtc_agent_amd import ops  # noqa: E402
from ai_rtc_agent_amd.config import sd_turbo_config  # noqa: E402
from ai_rtc_agent_amd.engine import StreamDiffusionEngine  # noqa: E402


def graph_time_us(fn, calls=20, reps=30):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / calls)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def bench_kernel():
    Bt, R, n = 8, 32, 4
    for L, K in ((4096, 320), (256, 1280)):
        N = K
        g = torch.Generator().manual_seed(0)
        h = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).half().cuda()
        x, y = h(Bt, L, K), h(Bt, L, N)
        A, B = h(n, R, K, sc=0.05), h(n, N, R, sc=0.05)
        ra = (torch.arange(Bt) % n).int().cuda()
        rs = torch.ones(Bt).cuda()
        idx = ra.long()
        sc = rs.view(-1, 1, 1).half()

        def kernel():
            ops.lora_delta_(y, x, A, B, ra, rs)

        def unfused():
            t = torch.bmm(x, A[idx].transpose(1, 2))
            y.add_(torch.bmm(t, B[idx].transpose(1, 2)) * sc)

        k = graph_time_us(kernel)
        u = graph_time_us(unfused)
        print(json.dumps({
            "what": "lora_delta_ vs gather + 2 bmm + add", "L": L, "K": K,
            "N": N, "R": R, "rows": Bt,
            "kernel_us": {"median": round(k[0], 2), "min": round(k[1], 2), "max": round(k[2], 2)},
            "bmm_route_us": {"median": round(u[0], 2), "min": round(u[1], 2), "max": round(u[2], 2)},
            "kernel_over_bmm": round(k[0] / u[0], 3)}), flush=True)


def bench_engine(frames: int):
    fbs = 8
    frame = torch.randint(0, 256, (fbs, 512, 512, 3), dtype=torch.uint8, device="cuda")
    # (c) loads one random rank-32 adapter over every target into all four
    # bank indices: the cost does not depend on the values
    for case in ("a: lora_adapters=0", "b: capacity 4, no slot assigned",
                 "c: capacity 4, all 8 slots assigned (one rank-32 adapter "
                 "over every target, in all 4 indices)"):
        cap = 0 if case.startswith("a") else 4
        eng = StreamDiffusionEngine(sd_turbo_config(
            device="cuda", frame_buffer_size=fbs, lora_adapters=cap,
            lora_max_rank=32))
        eng.prepare()
        if case.startswith("c"):
            g = torch.Generator().manual_seed(1)
            sd = {}
            for path, t in eng._lora_bank.targets.items():
                o, i = t.shape
                sd[f"{path}.lora_down.weight"] = torch.randn(32, i, generator=g) * 0.01
                sd[f"{path}.lora_up.weight"] = torch.randn(o, 32, generator=g) * 0.01
            for k in range(4):
                eng.load_adapter(k, sd, name=f"s{k}")
            for s in range(fbs):
                eng.update_lora(adapter=s % 4, slot=s)
        for _ in range(20):
            eng(frame)
        eng.sync_output()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            eng(frame)
        eng.sync_output()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"case": case, "fbs": fbs, "calls": frames,
                          "ms_per_call": round(dt / frames * 1e3, 3),
                          "aggregate_fps": round(frames * fbs / dt, 1)}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--kernel", action="store_true")
    p.add_argument("--engine", action="store_true")
    p.add_argument("--frames", type=int, default=100)
    a = p.parse_args()
    if not (a.kernel or a.engine):
        a.kernel = a.engine = True
    assert torch.cuda.is_available(), "lora_bench needs a GPU"
    if a.kernel:
        bench_kernel()
    if a.engine:
        bench_engine(a.frames)
