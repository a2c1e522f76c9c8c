#!/usr/bin/env python3
"""Per-op microbenchmarks at the SD shapes the frame actually runs.

    python tools/kernel_bench.py [--iters 50]

Reports per-op time and effective TFLOP/s (or GB/s for memory-bound ops)
with within-process interleaved repeats (guide §5.4 rule 24). GPU only.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from ai_rtc_agent_amd import ops

CONV_SHAPES = [
    # (name, B, H, W, IC, OC, k, stride)   — SD-Turbo/TAESD frame shapes
    ("unet 64x64x320 3x3", 1, 64, 64, 320, 320, 3, 1),
    ("unet 32x32x640 3x3", 1, 32, 32, 640, 640, 3, 1),
    ("unet 16x16x1280 3x3", 1, 16, 16, 1280, 1280, 3, 1),
    ("unet 8x8x1280 3x3", 1, 8, 8, 1280, 1280, 3, 1),
    ("unet up 32x32 1920->640", 1, 32, 32, 1920, 640, 3, 1),
    ("taesd 512x512x64 3x3", 1, 512, 512, 64, 64, 3, 1),
    ("taesd 256x256x64 3x3", 1, 256, 256, 64, 64, 3, 1),
    ("down 64->32 s2", 1, 64, 64, 320, 320, 3, 2),
    ("proj 64x64 320->640 1x1", 1, 64, 64, 320, 640, 1, 1),
]

ATTN_SHAPES = [
    # (name, B, Lq, Lk, C, heads)
    ("self 4096 c320 h5 (sd21@64x64)", 1, 4096, 4096, 320, 5),
    ("self 1024 c640 h10", 1, 1024, 1024, 640, 10),
    ("self 256 c1280 h20", 1, 256, 256, 1280, 20),
    ("cross 4096x77 c320", 1, 4096, 77, 320, 5),
    ("cross 1024x77 c640", 1, 1024, 77, 640, 10),
]

LINEAR_RES_SHAPES = [
    # (M, N, K): every projection of the headline UNet (SD-Turbo 512x512,
    # batch 1) that closes with a residual add. K = N: attention
    # out-projections and proj_out; K = 4N: feed-forward out
    (4096, 320, 320), (4096, 320, 1280),
    (1024, 640, 640), (1024, 640, 2560),
    (256, 1280, 1280), (256, 1280, 5120),
    (64, 1280, 1280), (64, 1280, 5120),
]


def timeit(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def window_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def captured(fn, iters):
    """`iters` back-to-back calls of fn as one hipGraph: replaying it times
    the device work without the host's launch cost, as in the engine's
    captured frame."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    return graph.replay


def bench_linear_residual(iters, reps=9):
    """F.linear + aten add against the one-call hipBLASLt epilogue
    (ops.linear, AIRTC_LT_EPILOGUE): device events around `iters`
    back-to-back calls, `reps` windows per side, sides alternating; median
    and min..max per call. Two rows per shape: eager calls (at these sizes
    the host's launch cost bounds them) and the same calls replayed from a
    hipGraph (device time, what the captured frame pays)."""
    dev = "cuda"
    ext = ops.hip_ext()
    print("== linear + residual (pair = F.linear + aten add, fused = one "
          "hipBLASLt call: bias epilogue, C = residual, beta = 1) ==")
    print(f"  {'M x N x K':>18s} {'mode':>6s}  {'pair us (min..max)':>24s}  "
          f"{'fused us (min..max)':>24s}  fused/pair  verdict")
    for m, n, k in LINEAR_RES_SHAPES:
        g = torch.Generator().manual_seed(m + n + k)
        x = (torch.randn(1, m, k, generator=g) / k ** 0.5).half().to(dev)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).half().to(dev)
        bias = torch.randn(n, generator=g).half().to(dev)
        res = torch.randn(1, m, n, generator=g).half().to(dev)
        pair = lambda: F.linear(x, w, bias) + res
        fused = lambda: ext.linear_residual(x, w, bias, res)
        for fn in (pair, fused):
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        sides = {"eager": (pair, fused, iters),
                 "graph": (captured(pair, iters), captured(fused, iters), 1)}
        for mode, (fp, ff, calls) in sides.items():
            t_p, t_f = [], []
            for _ in range(reps):
                t_p.append(window_us(fp, calls) * calls / iters)
                t_f.append(window_us(ff, calls) * calls / iters)
            mp, mf = statistics.median(t_p), statistics.median(t_f)
            # slower only counts beyond the side's own min..max spread
            slower = mf - mp > max(t_f) - min(t_f)
            print(f"  {f'{m} x {n} x {k}':>18s} {mode:>6s}  "
                  f"{f'{mp:7.2f} ({min(t_p):.2f}..{max(t_p):.2f})':>24s}  "
                  f"{f'{mf:7.2f} ({min(t_f):.2f}..{max(t_f):.2f})':>24s}  "
                  f"{mf / mp:10.3f}  {'SLOWER' if slower else 'ok'}")


def bench_conv_operands(iters, reps=9):
    """Convs that read their operands in place against the kernels they
    replace: the 1x1 shortcut + conv2 pair against conv2 with a pointwise
    tail, upsample + conv against nearest-2x in the A-load, and the
    4-/3-channel conv_in layers on the per-pixel kernel (or the pad-to-32
    route) against the lanes-along-OC kernel. Same method as the linear
    rows: device events around `iters` back-to-back calls, `reps` windows
    per side, sides alternating; eager and replayed from a hipGraph."""
    dev = "cuda"

    def t(*shape, scale=1.0):
        return (torch.randn(*shape, device=dev) * scale).half()

    def with_env(name, val, fn):
        def run():
            os.environ[name] = val
            try:
                return fn()
            finally:
                os.environ.pop(name, None)
        return run

    cases = []
    # (1) resnet shortcut: hw, cin (the concatenated input), cout
    for hw, cin, cout in ((64, 960, 320), (32, 1920, 640), (16, 2560, 1280),
                          (8, 2560, 1280)):
        x, x2 = t(1, hw, hw, cout), t(1, hw, hw, cin)
        w, w2 = t(cout, cout, 3, 3, scale=0.02), t(cout, cin, 1, 1, scale=0.02)
        b, b2 = t(cout), t(cout)
        cb = t(1, cout)
        call = (lambda x=x, x2=x2, w=w, w2=w2, b=b, b2=b2, cb=cb:
                ops.conv2d_nhwc(x, w, b, channel_bias=cb, tail=(x2, w2, b2)))
        cases.append((f"shortcut {hw}x{hw} {cin}->{cout}",
                      with_env("AIRTC_CONV_TAIL", "0", call), call))
    # (2) upsample in front of a conv: source hw, channels
    for hw, c in ((256, 64), (32, 640)):
        x, w, b = t(1, hw, hw, c), t(c, c, 3, 3, scale=0.02), t(c)
        call = lambda x=x, w=w, b=b: ops.conv2d_nhwc(x, w, b, upsample2x=True)
        cases.append((f"upsample {hw}->{2 * hw} c{c}",
                      with_env("AIRTC_CONV_UP", "0", call),
                      with_env("AIRTC_CONV_UP", "1", call)))
    # (3) tiny-IC conv_in layers
    for hw, ic, oc in ((64, 4, 320), (64, 4, 64), (512, 3, 64)):
        x, w, b = t(1, hw, hw, ic), t(oc, ic, 3, 3, scale=0.1), t(oc)
        old = with_env("AIRTC_CONV_TINYIC", "0",
                       lambda x=x, w=w, b=b: ops.conv2d_nhwc(x, w, b))
        wt, b32 = ops.interface._tiny_pack(w), b.float()
        ext = ops.hip_ext()
        new = (lambda x=x, wt=wt, b32=b32:
               ext.conv2d_tinyic(x=x, w_tiny=wt, bias=b32, R=3, S=3, stride=1,
                                 pad=1))
        cases.append((f"conv_in {hw}x{hw} {ic}->{oc}", old, new))

    print("== conv operands in place (old = the kernels replaced, new = one "
          "conv call) ==")
    print(f"  {'case':>28s} {'mode':>6s}  {'old us (min..max)':>24s}  "
          f"{'new us (min..max)':>24s}  new/old  verdict")
    for name, old, new in cases:
        for fn in (old, new):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        sides = {"eager": (old, new, iters),
                 "graph": (captured(old, iters), captured(new, iters), 1)}
        for mode, (fo, fn_, calls) in sides.items():
            t_o, t_n = [], []
            for _ in range(reps):
                t_o.append(window_us(fo, calls) * calls / iters)
                t_n.append(window_us(fn_, calls) * calls / iters)
            mo, mn = statistics.median(t_o), statistics.median(t_n)
            spread = max(max(t_o) - min(t_o), max(t_n) - min(t_n))
            verdict = ("faster" if mo - mn > spread
                       else "SLOWER" if mn - mo > spread else "same")
            print(f"  {name:>28s} {mode:>6s}  "
                  f"{f'{mo:7.2f} ({min(t_o):.2f}..{max(t_o):.2f})':>24s}  "
                  f"{f'{mn:7.2f} ({min(t_n):.2f}..{max(t_n):.2f})':>24s}  "
                  f"{mn / mo:7.3f}  {verdict}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--batch", type=int, default=1,
                   help="scale conv batch (the fbs>1 serving tier)")
    p.add_argument("--only", choices=["linear", "operands"],
                   help="run one group: linear = linear + residual, "
                        "operands = convs reading shortcut / upsample / "
                        "tiny-IC inputs in place")
    args = p.parse_args()
    assert torch.cuda.is_available(), "GPU microbench"
    dev = "cuda"
    if args.only == "linear":
        bench_linear_residual(max(args.iters, 200))
        return
    if args.only == "operands":
        bench_conv_operands(max(args.iters, 100))
        return

    print(f"== conv2d (NHWC implicit-GEMM MFMA) B={args.batch} ==")
    for name, b0, h, w, ic, oc, k, st in CONV_SHAPES:
        b = b0 * args.batch
        x = torch.randn(b, h, w, ic, device=dev).half()
        wt = (torch.randn(oc, ic, k, k, device=dev) * 0.02).half()
        bias = torch.randn(oc, device=dev).half()
        pad = k // 2
        fn = lambda: ops.conv2d_nhwc(x, wt, bias, stride=st, padding=pad)
        us = timeit(fn, args.iters)
        ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
        fl = 2.0 * b * ho * wo * oc * ic * k * k
        print(f"  {name:32s} {us:8.1f} us  {fl/us/1e6:7.1f} TF/s")

    print(f"== conv2d fp8 (MX-scaled MFMA, per-OC weight scales) B={args.batch} ==")
    for name, b0, h, w, ic, oc, k, st in CONV_SHAPES:
        if ic % 64 != 0:
            continue
        b = b0 * args.batch
        x = torch.randn(b, h, w, ic, device=dev).half()
        wt = (torch.randn(oc, ic, k, k, device=dev) * 0.02).half()
        bias = torch.randn(oc, device=dev).float()
        pad = k // 2
        a_scale = x.float().abs().max().item() / ops.FP8_MAX
        fn = lambda: ops.conv2d_fp8_nhwc(x, wt, a_scale, None, stride=st,
                                         padding=pad)
        us = timeit(fn, args.iters)
        ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
        fl = 2.0 * b * ho * wo * oc * ic * k * k
        print(f"  {name:32s} {us:8.1f} us  {fl/us/1e6:7.1f} TF/s")

    print(f"== conv2d fp8 pre-quantized input (GN-fp8 -> conv) B={args.batch} ==")
    for name, b0, h, w, ic, oc, k, st in CONV_SHAPES:
        if ic % 64 != 0:
            continue
        b = b0 * args.batch
        x = torch.randn(b, h, w, ic, device=dev).half()
        wt = (torch.randn(oc, ic, k, k, device=dev) * 0.02).half()
        pad = k // 2
        a_scale = x.float().abs().max().item() / ops.FP8_MAX
        xq = ((x.float() / a_scale).clamp(-448, 448)
              .to(torch.float8_e4m3fn).view(torch.uint8).contiguous())
        fn = lambda: ops.conv2d_fp8_nhwc(xq, wt, a_scale, None, stride=st,
                                         padding=pad)
        us = timeit(fn, args.iters)
        ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
        fl = 2.0 * b * ho * wo * oc * ic * k * k
        print(f"  {name:32s} {us:8.1f} us  {fl/us/1e6:7.1f} TF/s")

    print(f"== attention (flash MFMA + tr_b16) B={args.batch} ==")
    for name, b0, lq, lk, c, hds in ATTN_SHAPES:
        b = b0 * args.batch
        q = torch.randn(b, lq, c, device=dev).half()
        kk = torch.randn(b, lk, c, device=dev).half()
        v = torch.randn(b, lk, c, device=dev).half()
        fn = lambda: ops.attention(q, kk, v, hds)
        us = timeit(fn, args.iters)
        fl = 2.0 * 2 * b * lq * lk * c
        print(f"  {name:32s} {us:8.1f} us  {fl/us/1e6:7.1f} TF/s")

    print("== norms / elementwise (GB/s = read+write traffic) ==")
    x = torch.randn(1, 64, 64, 320, device=dev).half()
    g = torch.randn(320, device=dev).float()
    be = torch.randn(320, device=dev).float()
    us = timeit(lambda: ops.group_norm_silu_nhwc(x, 32, g, be), args.iters)
    traffic = x.numel() * 2 * 3  # 2 reads (stats+apply) + 1 write
    print(f"  {'group_norm_silu 64x64x320':32s} {us:8.1f} us  {traffic/us/1e3:7.1f} GB/s")

    # the conv -> GroupNorm chain with and without the statistics fused into
    # the split-K finalize. The finalize has no entry point of its own: its
    # cost is the difference of the two conv rows (plain vs stats), and its
    # absolute time is in the kernel-trace profiles
    # (profiles/kernel_time_rounds.md). The statistics are opt-in and read
    # per call; only the calls that pass stats_groups see the switch.
    os.environ["AIRTC_FIN_STATS"] = "1"
    print("== conv -> GroupNorm chain (fused = finalize emits the statistics) ==")
    for h, c in ((64, 320), (32, 640), (16, 1280)):
        xc = torch.randn(1, h, h, c, device=dev).half()
        wt = (torch.randn(c, c, 3, 3, device=dev) * 0.02).half()
        cb = torch.randn(1, c, device=dev).half()
        gc = torch.randn(c, device=dev).float()
        bc = torch.randn(c, device=dev).float()
        y_plain = ops.conv2d_nhwc(xc, wt, None, channel_bias=cb)
        y_stats = ops.conv2d_nhwc(xc, wt, None, channel_bias=cb, stats_groups=32)
        fused_ok = hasattr(y_stats, "_airtc_gn_part")
        rows = [
            ("conv+finalize", lambda: ops.conv2d_nhwc(xc, wt, None, channel_bias=cb)),
            ("conv+finalize(stats)", lambda: ops.conv2d_nhwc(
                xc, wt, None, channel_bias=cb, stats_groups=32)),
            ("gn stats+apply", lambda: ops.group_norm_silu_nhwc(y_plain, 32, gc, bc)),
            ("gn apply only", lambda: ops.group_norm_silu_nhwc(y_stats, 32, gc, bc)),
            ("chain unfused", lambda: ops.group_norm_silu_nhwc(
                ops.conv2d_nhwc(xc, wt, None, channel_bias=cb), 32, gc, bc)),
            ("chain fused", lambda: ops.group_norm_silu_nhwc(
                ops.conv2d_nhwc(xc, wt, None, channel_bias=cb, stats_groups=32),
                32, gc, bc)),
        ]
        # interleaved repeats: every row is timed in each of 3 rounds
        best = {n: float("inf") for n, _ in rows}
        for _ in range(3):
            for n, fn in rows:
                best[n] = min(best[n], timeit(fn, args.iters))
        if not fused_ok:
            print(f"  ({h}x{h}x{c}: the conv attached no partials)")
        for n, _ in rows:
            print(f"  {n + f' {h}x{h}x{c}':36s} {best[n]:8.1f} us")
    t = torch.randn(1, 4096, 320, device=dev).half()
    us = timeit(lambda: ops.layer_norm(t, g, be), args.iters)
    print(f"  {'layer_norm 4096x320':32s} {us:8.1f} us  {t.numel()*2*2/us/1e3:7.1f} GB/s")
    u8 = torch.randint(0, 256, (1, 512, 512, 3), dtype=torch.uint8, device=dev)
    us = timeit(lambda: ops.preprocess_from_u8(u8, torch.float16), args.iters)
    print(f"  {'preprocess 512x512':32s} {us:8.1f} us  {u8.numel()*3/us/1e3:7.1f} GB/s")

    bench_linear_residual(max(args.iters, 200))
    bench_conv_operands(max(args.iters, 100))


if __name__ == "__main__":
    main()
